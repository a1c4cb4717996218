"""Gradients with respect to the face crops (saliency, FGSM / PGD): the stem data-gradient kernel (csrc/stem_dgrad.hip) against fp64
autograd, then EfficientNet-B0, Xception and whole clips (harness.input_gradient) against the CPU oracle in fp64.

Gates.  The kernel: GRAD_TOL_UNIT.  A network: max(GRAD_TOL_UNIT, 3 x the fp32 oracle's own distance from the fp64 oracle on the same
inputs), computed here -- the same arithmetic in fp32 is the yardstick for what fp32 can give (measured on the CPU: 1.0e-5 / 1.2e-5
for EfficientNet eval / train, 1.2e-4 for a whole eval-extractor clip).  Xception (ReLU / max-pool mask flips; relative L2 as in
test_gpu_xception.test_all_parameter_gradients_vs_oracle): 3 REL_TOL + 3 x the fp32 oracle's relative L2 (6.1e-3 / 6.7e-3).
A train-mode-extractor clip is not gated: BatchNorm over 16 crops is ill-conditioned, the fp32 oracle itself is 1.4e-2 away."""
import functools

import pytest
import torch
import torch.nn.functional as F

import mintime_amd
from mintime_amd import harness, plans, synth, xception, EfficientNet
from mintime_amd import lib as L
from oracle import mintime_oracle as O
from tests.util import GRAD_TOL_UNIT, REL_TOL, rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture
def det_mode():
    prev = L.set_deterministic(True)
    yield
    L.set_deterministic(prev)


@pytest.fixture
def plan_switch():
    prev = plans.ENABLED
    yield
    plans.ENABLED = prev


# ---- the kernel ---------------------------------------------------------------------------------------------------------------

def _geometry(H, W, valid):
    Ho, Wo = ((H - 3) // 2 + 1, (W - 3) // 2 + 1) if valid else ((H + 1) // 2, (W + 1) // 2)
    pt_h = 0 if valid else max((Ho - 1) * 2 + 3 - H, 0)
    pt_w = 0 if valid else max((Wo - 1) * 2 + 3 - W, 0)
    return Ho, Wo, pt_h, pt_w


def _kernel_case(H, W, valid, N=2):
    Ho, Wo, pt_h, pt_w = _geometry(H, W, valid)
    g = torch.Generator().manual_seed(1000 * H + W + (7 if valid else 0))
    du = torch.randn(N * Ho * Wo, 32, generator=g)
    z = torch.randn(N * Ho * Wo, 32, generator=g)
    kabc = torch.rand(3, 32, generator=g) + 0.5
    w = torch.randn(32, 3, 3, 3, generator=g)
    # reference: fp64 autograd through F.conv2d of a zero input with the explicit TF padding
    dz = kabc[0].double() * du.double() + kabc[1].double() * z.double() + kabc[2].double()
    x = torch.zeros(N, 3, H, W, dtype=torch.float64, requires_grad=True)
    xp = F.pad(x, (pt_w // 2, pt_w - pt_w // 2, pt_h // 2, pt_h - pt_h // 2))
    y = F.conv2d(xp, w.double(), stride=2)
    assert y.shape == (N, 32, Ho, Wo)
    y.backward(dz.view(N, Ho, Wo, 32).permute(0, 3, 1, 2))
    return du, z, kabc, w, x.grad.permute(0, 2, 3, 1).contiguous()


def _launch(du, z, kabc, w, N, H, W, valid):
    lib = L.get()
    fn = lib.mt_stem_conv_dgrad_valid if valid else lib.mt_stem_conv_dgrad
    dx = torch.full((N, H, W, 3), float("nan"), device="cuda")
    rc = fn(L.ptr(du), L.ptr(z), L.ptr(kabc), L.ptr(w), L.ptr(dx), N, H, W, L.stream_ptr())
    torch.cuda.synchronize()
    return rc, dx


# the last SAME / valid shape of each list: more than one run of rows per image (a run re-computes the output row above it)
@pytest.mark.parametrize("H,W,valid", [(8, 12, False), (9, 13, False), (6, 224, False), (5, 301, False), (4, 512, False), (40, 36, False),
                                       (3, 3, True), (8, 8, True), (9, 11, True), (7, 299, True), (37, 40, True)])
def test_stem_dgrad_kernel_matches_fp64_autograd(H, W, valid):
    N = 2
    du, z, kabc, w, ref = _kernel_case(H, W, valid, N)
    dev = [t.cuda() for t in (du, z, kabc, w)]
    outs = []
    prev = L.deterministic()
    try:
        for det in (False, True, False, True):
            L.set_deterministic(det)
            rc, dx = _launch(*dev, N, H, W, valid)
            assert rc == 0, L.get().mt_last_error()
            outs.append(dx)
    finally:
        L.set_deterministic(prev)
    assert bool(torch.isfinite(outs[0]).all())                   # every element written (the buffer was NaN)
    err = rel_err(outs[0], ref)
    print(f"stem dgrad {'valid' if valid else 'same'} {H}x{W}: rel err {err:.2e}")
    assert err <= GRAD_TOL_UNIT
    for o in outs[1:]:
        assert torch.equal(o, outs[0])                           # no atomics: the same bits every launch, in either mode
    if valid and H % 2 == 0:
        assert float(outs[0][:, H - 1].abs().max()) == 0.0       # no tap reaches the last row / column of an even size
    if valid and W % 2 == 0:
        assert float(outs[0][:, :, W - 1].abs().max()) == 0.0


@pytest.mark.parametrize("H,W,valid", [(8, 513, False), (8, 9, False), (2, 8, True), (8, 2, True), (8, 513, True)])
def test_stem_dgrad_refuses_what_the_forward_refuses(H, W, valid):
    """Crops wider than the LDS row tile, H and W with different leading pads (8 -> 0, 9 -> 1), valid padding below 3 x 3: an error
    code, and no launch (the output keeps its fill)."""
    N = 1
    du = torch.zeros(N * 8 * 300, 32, device="cuda")
    kabc = torch.ones(3, 32, device="cuda")
    w = torch.ones(32, 3, 3, 3, device="cuda")
    rc, dx = _launch(du, du, kabc, w, N, H, W, valid)
    assert rc != 0 and L.get().mt_last_error()
    assert bool(torch.isnan(dx).all())


# ---- EfficientNet-B0 ------------------------------------------------------------------------------------------------------------

def _ef_model(seed, training):
    m = EfficientNet.from_name("efficientnet-b0", drop_connect_rate=0.0)
    sd = synth.effnet_b0_state(seed)
    m.load_state_dict(sd, strict=True)
    m.train(training)
    return m.cuda(), sd


def _gate(floor):
    return max(GRAD_TOL_UNIT, 3.0 * floor)


@functools.lru_cache(maxsize=None)
def _ef_reference(training):
    """(crops [n,224,224,3], loss weights, d loss / d crops in fp64 [n,224,224,3], fp32-oracle floor); computed once, never modified."""
    seed, n = 3, 2
    sd = synth.effnet_b0_state(seed)
    v = synth.clip_inputs(1, n, 1, seed)["videos"].reshape(n, 224, 224, 3)
    wts = torch.randn(n, 1280, 7, 7, generator=torch.Generator().manual_seed(21)) * 0.1
    grads = []
    for dt in (torch.float64, torch.float32):
        leaf = v.to(dt, copy=True).requires_grad_(True)
        feat = O.effnet_b0_forward(O.to_dtype(sd, dt), leaf.permute(0, 3, 1, 2), training=training)
        (feat * wts.to(dt)).sum().backward()
        grads.append(leaf.grad.detach())
    return v, wts, grads[0], rel_err(grads[1], grads[0])


@pytest.mark.parametrize("training,layout", [(False, "nhwc"), (True, "nhwc"), (False, "nchw")])
def test_effnet_crop_gradient_vs_fp64_oracle(training, layout):
    """x.requires_grad_() through autograd: the NHWC-strided view of train.py:341 and a plain contiguous NCHW tensor."""
    v, wts, ref, floor = _ef_reference(training)
    model, _ = _ef_model(3, training)
    if layout == "nhwc":
        leaf = v.cuda().requires_grad_(True)
        x = leaf.permute(0, 3, 1, 2)
    else:
        leaf = v.permute(0, 3, 1, 2).contiguous().cuda().requires_grad_(True)
        x = leaf
    feat = model(x)
    (feat * wts.cuda()).sum().backward()
    got = leaf.grad if layout == "nhwc" else leaf.grad.permute(0, 2, 3, 1)
    assert got.shape == ref.shape and got.dtype == torch.float32
    err = rel_err(got, ref)
    print(f"effnet d/d crops ({'train' if training else 'eval'}, {layout}): ours {err:.2e}, fp32 oracle {floor:.2e}, gate {_gate(floor):.2e}")
    assert err <= _gate(floor)
    assert all(p.grad is not None for k, p in model.named_parameters() if not k.startswith("_fc"))


def _unfreeze_rule(named_params, unfreeze_blocks):
    """train.py:157-170 (as tests/test_gpu_e2e.py states it): only MBConv blocks >= 16 - k stay trainable."""
    for name, p in named_params:
        p.requires_grad_("blocks" in name and int(name.split(".")[1]) >= 16 - unfreeze_blocks)


@pytest.mark.parametrize("config", ["all_trainable", "all_frozen_eval", "unfreeze_3"])
def test_crop_gradient_reaches_the_stem_whatever_is_frozen(config, det_mode):
    """The walk reaches the stem through frozen blocks, frozen parameters get no gradient, and (deterministic mode) the trainable ones
    get the bits they get without a gradient on the crops."""
    from mintime_amd import effnet_backward as EB
    training = config != "all_frozen_eval"
    v, wts, ref, floor = _ef_reference(training)
    runs = []
    for with_dx in (True, False):
        model, _ = _ef_model(3, training)
        if config == "all_frozen_eval":
            for p in model.parameters():
                p.requires_grad_(False)
        elif config == "unfreeze_3":
            _unfreeze_rule(model.named_parameters(), 3)
        trainable = [k for k, p in model.named_parameters() if p.requires_grad and not k.startswith("_fc")]
        if not with_dx and not trainable:
            break                                                # nothing requires grad: there is no backward to compare with
        leaf = v.cuda().requires_grad_(with_dx)
        feat = model(leaf.permute(0, 3, 1, 2))
        (feat * wts.cuda()).sum().backward()
        for k, p in model.named_parameters():
            assert (p.grad is not None) == (k in trainable), k
        if with_dx:
            err = rel_err(leaf.grad, ref)
            print(f"{config}: d/d crops {err:.2e} (fp32 oracle {floor:.2e})")
            assert err <= _gate(floor)
            assert EB.LAST_RUN["blocks_run"] == 16 and EB.LAST_RUN["stem_run"] is True
        runs.append({k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None})
    if len(runs) == 2:
        assert runs[0].keys() == runs[1].keys()
        diff = [k for k in runs[0] if not torch.equal(runs[0][k], runs[1][k])]
        assert not diff, f"{len(diff)} parameter gradients changed with requires_grad on the crops, e.g. {diff[:4]}"


# ---- Xception -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("training", [False, True])
def test_xception_crop_gradient_vs_fp64_oracle(training):
    seed, n = 4, 2
    sd = synth.xception_state(seed)
    v = synth.clip_inputs(1, n, 1, seed)["videos"].reshape(n, 224, 224, 3)
    wts = torch.randn(n, 2048, 7, 7, generator=torch.Generator().manual_seed(3)) * 0.1
    grads = []
    for dt in (torch.float64, torch.float32):
        leaf = v.to(dt, copy=True).requires_grad_(True)
        (O.xception_forward(O.to_dtype(sd, dt), leaf.permute(0, 3, 1, 2), training=training) * wts.to(dt)).sum().backward()
        grads.append(leaf.grad.detach())
    ref = grads[0]
    model = xception(num_classes=1, pretrain_path=None)
    model.load_state_dict(sd, strict=True)
    model.train(training).cuda()
    leaf = v.cuda().requires_grad_(True)
    (model(leaf.permute(0, 3, 1, 2)) * wts.cuda()).sum().backward()
    assert leaf.grad.shape == ref.shape
    rl2 = lambda a: float((a.detach().cpu().double() - ref).norm() / ref.norm())
    floor, ours = rl2(grads[1]), rl2(leaf.grad)
    print(f"xception d/d crops ({'train' if training else 'eval'}): ours {ours:.2e}, fp32 oracle {floor:.2e}")
    assert ours <= 3 * REL_TOL + 3 * floor
    # last row / column of the even-sized crop: no tap of the unpadded stride-2 conv1 reaches them
    assert float(leaf.grad[:, 223].abs().max()) == 0.0 and float(leaf.grad[:, :, 223].abs().max()) == 0.0


# ---- whole clips ------------------------------------------------------------------------------------------------------------------

def _to_device(inp):
    return {k: (t.cuda() if k != "size_embedding" else t) for k, t in inp.items()}


@pytest.mark.parametrize("B", [1, 2])
def test_clip_crop_gradient_vs_fp64_oracle(B):
    """Eval extractor, ragged clips.  B = 1: the saliency setting (both modules eval(), every parameter frozen), legacy TimeSformer
    engine; B = 2: trainable TimeSformer in train mode, plane path."""
    seed, Fr = 7, 8
    cfg, ef, tsf = harness.build_models(Fr, seed=seed, device="cuda", drop_connect_rate=0.0, train_extractor=False)
    if B == 1:
        tsf.eval()
        for p in list(ef.parameters()) + list(tsf.parameters()):
            p.requires_grad_(False)
    inp = synth.clip_inputs(B, Fr, 2, seed, ragged=True)
    grads = []
    for dt in (torch.float64, torch.float32):
        leaf = inp["videos"].to(dt, copy=True).requires_grad_(True)
        yo = O.clip_forward(O.to_dtype(synth.effnet_b0_state(seed), dt), O.to_dtype(synth.tsf_state(cfg, seed), dt), cfg,
                            dict(inp, videos=leaf), training_extractor=False)
        lo = O.bce_with_logits(yo, inp["labels"])
        lo.backward()
        grads.append(leaf.grad.detach())
        if dt == torch.float64:
            ylog, loss64 = yo.detach(), lo.detach()
    ref, floor = grads[0], rel_err(grads[1], grads[0])
    masked = ~inp["mask"]
    assert float(ref[masked].abs().max()) == 0.0                  # the oracle: padded slots get no gradient at all
    logits, loss, dv = harness.input_gradient(ef, tsf, _to_device(inp))
    assert dv.shape == inp["videos"].shape and dv.dtype == torch.float32
    assert rel_err(logits, ylog) <= REL_TOL and rel_err(loss, loss64) <= REL_TOL
    err = rel_err(dv, ref)
    print(f"clip d/d videos (B = {B}): ours {err:.2e}, fp32 oracle {floor:.2e}, gate {_gate(floor):.2e}")
    assert err <= _gate(floor)
    assert float(dv[masked.cuda()].abs().max()) <= 1e-6 * float(dv.abs().max())
    assert all(p.grad is None for p in list(ef.parameters()) + list(tsf.parameters()))


def test_baseline_clip_crop_gradient_vs_fp64():
    """--model 0: one clip of two frames through EfficientNet-B0 (eval) and the Baseline head, frame-averaged logit."""
    seed, Fr = 2, 2
    cfg, ex, model = harness.build_baseline(Fr, seed=seed, device="cuda", extractor=0, drop_connect_rate=0.0, train_extractor=False)
    inp = synth.clip_inputs(1, Fr, 1, seed)
    hs = synth.baseline_state(cfg, seed)
    grads = []
    for dt in (torch.float64, torch.float32):
        leaf = inp["videos"].to(dt, copy=True).requires_grad_(True)
        feat = O.effnet_b0_forward(O.to_dtype(synth.effnet_b0_state(seed), dt), leaf.reshape(Fr, 224, 224, 3).permute(0, 3, 1, 2),
                                   training=False)
        h = F.linear(feat.mean(dim=(2, 3)), hs["mlp_head.0.weight"].to(dt), hs["mlp_head.0.bias"].to(dt))      # baseline.py:31-36
        y = F.linear(h, hs["mlp_head.1.weight"].to(dt), hs["mlp_head.1.bias"].to(dt))
        yo = torch.mean(y.reshape(-1, Fr), 1).unsqueeze(1)                                                       # train.py:352
        O.bce_with_logits(yo, inp["labels"]).backward()
        grads.append(leaf.grad.detach())
        if dt == torch.float64:
            ylog = yo.detach()
    ref, floor = grads[0], rel_err(grads[1], grads[0])
    logits, loss, dv = harness.input_gradient(ex, model, _to_device(inp))
    assert dv.shape == inp["videos"].shape
    assert rel_err(logits, ylog) <= REL_TOL
    err = rel_err(dv, ref)
    print(f"baseline clip d/d videos: ours {err:.2e}, fp32 oracle {floor:.2e}, gate {_gate(floor):.2e}")
    assert err <= _gate(floor)


# ---- launch plans -------------------------------------------------------------------------------------------------------------------

def _plan_entries(*modules):
    return sum(len(plans._REG.get(m, {})) for m in modules)


def _steps(with_input_gradient):
    cfg, ef, tsf = harness.build_models(8, seed=4, device="cuda", drop_connect_rate=0.0)
    opt = harness.make_optimizer(cfg, ef, tsf)
    batches = [harness.device_batch(2, 8, 2, seed=i, device="cuda", ragged=i % 2 == 1) for i in range(4)]
    out = None
    for i, batch in enumerate(batches):
        if i == 3 and with_input_gradient:
            entries, recorded = _plan_entries(ef, tsf), plans.STATS["recorded"]
            _, _, dv = harness.input_gradient(ef, tsf, batches[1])
            assert bool(torch.isfinite(dv).all()) and float(dv.abs().max()) > 0
            assert _plan_entries(ef, tsf) == entries and plans.STATS["recorded"] == recorded
        logits = harness.forward(ef, tsf, batch)
        loss = mintime_amd.optim.bce_with_logits(logits, batch["labels"], None)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        out = (logits.detach().clone(), {k: p.grad.detach().clone() for m in (ef, tsf) for k, p in m.named_parameters() if p.grad is not None})
        opt.step()
    torch.cuda.synchronize()
    return out


def test_input_gradient_between_planned_steps_leaves_them_alone(det_mode, plan_switch):
    """Three planned training steps, one input_gradient call, one more step: the last step's logits and gradients are the bits of
    four plain steps, and the call neither used nor added a launch plan of the extractor."""
    plans.ENABLED = True
    replayed = plans.STATS["replayed"]
    logits_a, grads_a = _steps(True)
    assert plans.STATS["replayed"] > replayed                    # the steps around the call did run from plans
    logits_b, grads_b = _steps(False)
    assert torch.equal(logits_a, logits_b)
    assert grads_a.keys() == grads_b.keys()
    diff = [k for k in grads_a if not torch.equal(grads_a[k], grads_b[k])]
    assert not diff, f"{len(diff)} gradients differ after an input_gradient call between planned steps, e.g. {diff[:4]}"
