"""GPU parity of the Baseline model (`--model 0`: reference models/baseline.py, train.py:341-352, test.py:238-244) on the HIP head
(include/mintime_hip.h "Baseline head"): against the imported reference's fixtures (tools/make_golden.py GOLDEN_ONLY=baseline) and
against float64 torch statements of the head computed here."""
import numpy as np
import pytest
import torch

import mintime_amd
from mintime_amd import arch, harness, optim, synth
from mintime_amd import baseline as BL
from tests.util import GRAD_TOL_UNIT, REL_TOL, assert_close, checksum, golden, probe_vector

pytestmark = pytest.mark.gpu

GRAD_TOL_EF = 6e-4      # test_gpu_e2e.py's gate of EfficientNet parameter gradients; each gradient here also gets 2x its fp32 floor


def _head_model(cfg, seed):
    m = mintime_amd.Baseline(cfg)
    m.load_state_dict(synth.baseline_state(cfg, seed))
    return m.cuda().train()


def _fixture_features(g, layout, requires_grad=True):
    """The fixture's seeded features on the device: NHWC storage seen as [n, C, 7, 7] (the extractors' output) or NCHW-contiguous."""
    clips, frames, C = int(g["clips"]), int(g["frames"]), int(g["channels"])
    f = synth.features(clips, frames, C, int(g["seed"]))
    f = f.reshape(clips * frames, *f.shape[2:])
    assert abs(checksum(f) - float(g["input_sum"])) <= 1e-9 * abs(float(g["input_sum"]))
    if layout == "nhwc":
        x = f.permute(0, 2, 3, 1).contiguous().cuda().permute(0, 3, 1, 2)
        assert x.permute(0, 2, 3, 1).is_contiguous() and not x.is_contiguous()
    else:
        x = f.contiguous().cuda()
    return x.detach().requires_grad_(requires_grad)


def _head_step(m, x, labels, frames):
    y = m(x)
    yc = torch.mean(y.reshape(-1, frames), 1).unsqueeze(1)            # train.py:352
    loss = optim.bce_with_logits(yc, labels)
    loss.backward()
    return y, loss


def _check_head_grads(m, g, suffix="64", tol=GRAD_TOL_UNIT, what=""):
    named = dict(m.named_parameters())
    for key in ("mlp_head.0.bias", "mlp_head.1.weight", "mlp_head.1.bias"):
        assert_close(named[key].grad, g[f"g{suffix}.{key}"], tol, f"{what} grad {key}")
    gw = named["mlp_head.0.weight"].grad.detach()
    assert_close(gw[::16], g[f"grows{suffix}.mlp_head.0.weight"], tol, f"{what} grad mlp_head.0.weight (every 16th row)")
    ref_norm = float(g[f"gnorm{suffix}.mlp_head.0.weight"])
    got = gw.double().cpu().reshape(-1)
    assert abs(float(got.norm()) - ref_norm) <= tol * ref_norm
    r = torch.from_numpy(probe_vector("mlp_head.0.weight", got.numel(), int(g["seed"])))
    assert abs(float((got * r).sum()) - float(g[f"gdot{suffix}.mlp_head.0.weight"])) <= tol * 0.57735 * ref_norm


@pytest.mark.parametrize("layout", ["nhwc", "nchw"])
def test_head_matches_reference_fixture(layout):
    g = golden("baseline_head")
    cfg = arch.default_baseline_config(int(g["channels"]), int(g["frames"]))
    sd = synth.baseline_state(cfg, int(g["seed"]))
    assert abs(checksum(sd["mlp_head.0.weight"]) - float(g["w1_sum"])) <= 1e-9 * abs(float(g["w1_sum"]))
    for k in ("mlp_head.0.bias", "mlp_head.1.weight", "mlp_head.1.bias"):
        assert np.array_equal(sd[k].numpy(), g["w." + k])
    m = _head_model(cfg, int(g["seed"]))
    x = _fixture_features(g, layout)
    y, loss = _head_step(m, x, torch.from_numpy(g["labels"]).cuda(), int(g["frames"]))
    assert y.shape == (x.shape[0], 1)
    assert_close(y, g["logits64"], REL_TOL, "logits")
    assert_close(loss, g["loss64"], REL_TOL, "loss")
    _check_head_grads(m, g, what=layout)
    # the input gradient: in the input's own layout, every pixel = the reference's (AdaptiveAvgPool2d spreads it evenly)
    assert x.grad is not None and x.grad.stride() == x.stride(), (x.grad.stride(), x.stride())
    want = torch.from_numpy(g["gx64"])[:, :, None, None].expand(x.shape)
    assert_close(x.grad, want, GRAD_TOL_UNIT, f"input gradient ({layout})")
    assert BL.LAST_RUN == {"param_grads": True, "dfeat": True}


def _cuda_batch(inp):
    return {k: (v.cuda() if k != "size_embedding" else v) for k, v in inp.items()}


def test_effnet_baseline_train_step_matches_reference_fixture():
    """`--model 0` with EfficientNet-B0 in train mode (drop-connect 0): clip logits, loss, running statistics and every gradient of
    both networks against the reference's float64 step."""
    g = golden("baseline_e2e_train")
    B, Fr, seed = int(g["batch"]), int(g["frames"]), int(g["seed"])
    cfg, ef, head = harness.build_baseline(num_frames=Fr, seed=seed, extractor=0, drop_connect_rate=0.0)
    inp = synth.clip_inputs(B, Fr, 1, seed)
    assert abs(checksum(inp["videos"]) - float(g["input_sum"])) <= 1e-9 * abs(float(g["input_sum"]))
    batch = _cuda_batch(inp)
    yc = harness.baseline_forward(ef, head, batch)
    loss = optim.bce_with_logits(yc, batch["labels"])
    loss.backward()
    assert yc.shape == (B, 1)
    assert_close(yc, g["clip_logits64"], REL_TOL, "clip logits")
    assert_close(loss, g["loss64"], REL_TOL, "loss")
    _check_head_grads(head, g, what="e2e")
    esd = ef.state_dict()
    for key in [k[len("stat64."):] for k in g.files if k.startswith("stat64.")]:
        assert_close(esd[key], g["stat64." + key], REL_TOL, "running statistic " + key)
    named = dict(ef.named_parameters())
    n = 0
    for key in [k[len("gnorm64.ef."):] for k in g.files if k.startswith("gnorm64.ef.")]:
        got = named[key].grad.detach().double().cpu().reshape(-1)
        ref_norm, ref_max = float(g["gnorm64.ef." + key]), float(g["gabsmax64.ef." + key])
        if key.endswith("_bn2.bias"):
            wn = float(named[key.replace(".bias", ".weight")].grad.norm())
            if ref_norm < 1e-3 * wn:                  # analytically zero under train-mode BatchNorm (see test_gpu_e2e.py)
                assert float(got.norm()) < 1e-3 * wn, key
                continue
        floor = float(g["gfloor." + key])
        tol = GRAD_TOL_EF + 2 * floor
        step = max(1, got.numel() // 256)
        err = float((got[::step][:256] - torch.from_numpy(g["gsample64.ef." + key])).abs().max()) / ref_max
        nerr = abs(float(got.norm()) - ref_norm) / ref_norm
        assert err <= tol and nerr <= tol, f"{key}: sample error {err:.2e}, norm error {nerr:.2e} (gate {tol:.2e})"
        r = torch.from_numpy(probe_vector("ef." + key, got.numel(), seed))
        cdot = abs(float((got * r).sum()) - float(g["gdot64.ef." + key])) / (0.57735 * ref_norm)
        assert cdot <= 8e-4 + 2 * floor, f"{key}: checksum sum(g*r) off by {cdot:.2e} |g|"
        n += 1
    assert n > 150


def _head64(m, feats, labels, frames):
    """The head in float64 torch (the reference's arithmetic): AdaptiveAvgPool2d(1), Linear, Linear, frame mean, BCE."""
    w1, b1, w2, b2 = (p.detach().double().requires_grad_(True) for p in m._param_list())
    f64 = feats.detach().double().requires_grad_(True)
    y = (f64.mean(dim=(2, 3)) @ w1.t() + b1) @ w2.t() + b2
    y.retain_grad()
    loss = torch.nn.functional.binary_cross_entropy_with_logits(torch.mean(y.reshape(-1, frames), 1).unsqueeze(1),
                                                                labels.double().reshape(-1, 1))
    loss.backward()
    return y, loss, f64, (w1, b1, w2, b2)


def test_xception_baseline_head_and_feature_gradient():
    """`--extractor_model 1`: Xception features (dim 2048) into the head; the head against a float64 statement of it on the same
    features, and the feature gradient Xception's backward receives = g_i v / hw, in the NHWC layout its engine wants (no copy)."""
    Fr, seed = 16, 5
    cfg, xc, head = harness.build_baseline(num_frames=Fr, seed=seed, extractor=1)
    batch = _cuda_batch(synth.clip_inputs(2, Fr, 1, seed))
    v = batch["videos"]
    feats = xc(v.reshape(-1, *v.shape[2:]).permute(0, 3, 1, 2))
    assert feats.shape == (2 * Fr, 2048, 7, 7)
    seen = {}
    feats.register_hook(lambda gr: seen.__setitem__("dfeat", gr))
    y = head(feats)
    loss = optim.bce_with_logits(torch.mean(y.reshape(-1, Fr), 1).unsqueeze(1), batch["labels"])
    loss.backward()
    y64, loss64, f64, p64 = _head64(head, feats, batch["labels"], Fr)
    assert_close(y, y64, REL_TOL, "logits")
    assert_close(loss, loss64, REL_TOL, "loss")
    for p, q in zip(head._param_list(), p64):
        assert_close(p.grad, q.grad, GRAD_TOL_UNIT, "head gradient " + str(tuple(p.shape)))
    d = seen["dfeat"]
    assert d.permute(0, 2, 3, 1).is_contiguous()              # autograd hands Xception's backward a contiguous [n*hw, C] buffer
    vvec = p64[0].detach().t() @ p64[2].detach().reshape(-1)   # v = W1^T w2
    want = (y64.grad.reshape(-1, 1) * vvec.reshape(1, -1) / 49.0)[:, :, None, None].expand(d.shape)
    assert_close(d, want, GRAD_TOL_UNIT, "dfeat = g v / hw")
    assert_close(d, f64.grad, GRAD_TOL_UNIT, "dfeat vs float64 autograd")
    assert all(bool(torch.isfinite(p.grad).all()) for p in xc.parameters() if p.grad is not None)
    # one training step through the harness (train.py:341-378)
    opt = harness.make_optimizer(cfg, xc, head)
    before = head.mlp_head._modules["0"].weight.detach().clone()
    step_loss = harness.baseline_train_step(xc, head, opt, batch)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(step_loss)) and not torch.equal(before, head.mlp_head._modules["0"].weight.detach())
    assert all(bool(torch.isfinite(p).all()) for p in list(xc.parameters()) + list(head.parameters()))


def test_frozen_backbone_and_frozen_parameters_launch_nothing_for_them():
    """--freeze_backbone (train.py:344-346): features without gradient -> head gradients as in the fixture and no input gradient; head
    parameters with requires_grad=False get none either."""
    g = golden("baseline_head")
    cfg = arch.default_baseline_config(int(g["channels"]), int(g["frames"]))
    m = _head_model(cfg, int(g["seed"]))
    x = _fixture_features(g, "nhwc", requires_grad=False)
    _head_step(m, x, torch.from_numpy(g["labels"]).cuda(), int(g["frames"]))
    assert BL.LAST_RUN == {"param_grads": True, "dfeat": False}
    _check_head_grads(m, g, what="frozen backbone")
    # only the input needs a gradient
    m2 = _head_model(cfg, int(g["seed"]))
    for p in m2.parameters():
        p.requires_grad_(False)
    x2 = _fixture_features(g, "nhwc")
    _head_step(m2, x2, torch.from_numpy(g["labels"]).cuda(), int(g["frames"]))
    assert BL.LAST_RUN == {"param_grads": False, "dfeat": True}
    assert all(p.grad is None for p in m2.parameters())
    assert_close(x2.grad, torch.from_numpy(g["gx64"])[:, :, None, None].expand(x2.shape), GRAD_TOL_UNIT, "input gradient")
    # the harness with the extractor frozen: EfficientNet in eval() under no_grad, only the head trains
    cfg3, ef, head = harness.build_baseline(num_frames=8, seed=2, extractor=0, train_extractor=False)
    opt = optim.FusedSGD(head.parameters(), lr=cfg3["training"]["lr"], weight_decay=cfg3["training"]["weight-decay"])
    loss = harness.baseline_train_step(ef, head, opt, _cuda_batch(synth.clip_inputs(1, 8, 1, 2)), freeze_backbone=True)
    assert bool(torch.isfinite(loss)) and all(p.grad is None for p in ef.parameters())
    assert BL.LAST_RUN == {"param_grads": True, "dfeat": False}


def test_gradients_bit_identical_run_to_run_and_large_batch_parity():
    """No atomics: two identical passes give the same bits.  n = 1024 crops x 2048 channels (config 5 at B = 64) crosses 2^28 elements
    of features and takes the multi-slab reduction; parity against float64 on the device."""
    g = golden("baseline_head")
    cfg = arch.default_baseline_config(int(g["channels"]), int(g["frames"]))
    runs = []
    for _ in range(2):
        m = _head_model(cfg, int(g["seed"]))
        x = _fixture_features(g, "nhwc")
        y, _ = _head_step(m, x, torch.from_numpy(g["labels"]).cuda(), int(g["frames"]))
        runs.append([y.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in m._param_list()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    n, C = 1024, 2048
    cfg = arch.default_baseline_config(C, 16)
    gen = torch.Generator(device="cuda").manual_seed(7)
    xb = torch.randn(n, 7, 7, C, device="cuda", generator=gen).clamp_min_(-0.3)
    gl = torch.randn(n, 1, device="cuda", generator=gen)
    outs = []
    for _ in range(2):
        m = _head_model(cfg, 9)
        x = xb.permute(0, 3, 1, 2).detach().requires_grad_(True)
        y = m(x)
        y.backward(gl)
        outs.append((y.detach(), x.grad, [p.grad for p in m._param_list()]))
        del x
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert all(torch.equal(a, b) for a, b in zip(outs[0][2], outs[1][2]))
    y, dx, grads = outs[0]
    w1, b1, w2, b2 = (p.detach().double().requires_grad_(True) for p in m._param_list())
    pooled = xb.double().mean(dim=(1, 2))
    y64 = (pooled @ w1.t() + b1) @ w2.t() + b2
    y64.backward(gl.double())
    assert_close(y, y64, REL_TOL, "logits (n = 1024)")
    for got, ref in zip(grads, (w1.grad, b1.grad, w2.grad, b2.grad)):
        assert_close(got, ref, GRAD_TOL_UNIT, "parameter gradient (n = 1024) " + str(tuple(ref.shape)))
    v64 = (w1.detach().t() @ w2.detach().reshape(-1))
    want = gl.double().reshape(n, 1) * v64.reshape(1, C) / 49.0                  # [n, C], the same at every pixel
    err = float((dx.double().permute(0, 2, 3, 1) - want[:, None, None, :]).abs().max()) / float(want.abs().max())
    assert err <= GRAD_TOL_UNIT, f"input gradient (n = 1024): {err:.2e}"


def test_second_backward_and_updated_weights_are_refused():
    g = golden("baseline_head")
    cfg = arch.default_baseline_config(int(g["channels"]), int(g["frames"]))
    m = _head_model(cfg, 1)
    x = _fixture_features(g, "nhwc")
    y = m(x)
    y.sum().backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="second time"):
        y.sum().backward()
    y = m(x)
    with torch.no_grad():
        m.mlp_head._modules["1"].weight.mul_(2.0)
    with pytest.raises(RuntimeError, match="updated between"):
        y.sum().backward()


def test_nn_dataparallel_wrap_on_one_gpu_is_transparent():
    """train.py / test.py wrap the model in nn.DataParallel: on one visible GPU forward, backward and the `module.` state-dict keys
    behave like the bare module."""
    g = golden("baseline_head")
    cfg = arch.default_baseline_config(int(g["channels"]), int(g["frames"]))
    labels = torch.from_numpy(g["labels"]).cuda()
    m0 = _head_model(cfg, int(g["seed"]))
    x0 = _fixture_features(g, "nhwc")
    y0, _ = _head_step(m0, x0, labels, int(g["frames"]))
    m1 = _head_model(cfg, int(g["seed"]))
    dp = torch.nn.DataParallel(m1, device_ids=[0])
    assert sorted(dp.state_dict()) == sorted("module." + k for k in m0.state_dict())
    x1 = _fixture_features(g, "nhwc")
    y1, _ = _head_step(dp, x1, labels, int(g["frames"]))
    assert_close(y1, y0, 1e-6, "logits through DataParallel")
    for p0, p1 in zip(m0._param_list(), m1._param_list()):
        assert torch.equal(p0.grad, p1.grad)
    assert torch.equal(x0.grad, x1.grad)
