"""The reference callers' step bodies (train.py:332-381, test.py:235-247) on the MI355X modules, for synthetic
inputs.  train.py / test.py themselves import tensorflow, cv2, albumentations, timm ... and cannot run offline;
this reproduces exactly what they do with the two models (same rearranges, same kwargs, same loss, same optimizer)."""
import torch
import torch.nn.functional as F

from . import arch, optim, synth
from .efficientnet import EfficientNet
from .timesformer import SizeInvariantTimeSformer
from .baseline import Baseline
from . import slowfast as _slowfast


def build_models(num_frames=8, seed=0, device="cuda", require_attention=False, drop_connect_rate=arch.DROP_CONNECT_RATE,
                 train_extractor=True):
    cfg = arch.default_tsf_config(1280, num_frames)
    ef = EfficientNet.from_name("efficientnet-b0", drop_connect_rate=drop_connect_rate)
    ef.load_state_dict(synth.effnet_b0_state(seed))
    tsf = SizeInvariantTimeSformer(config=cfg, require_attention=require_attention)
    tsf.load_state_dict(synth.tsf_state(cfg, seed))
    ef.to(device).train(train_extractor)
    tsf.to(device).train()
    return cfg, ef, tsf


def build_models_xs(num_frames=16, seed=0, device="cuda", require_attention=False):
    """BASELINE config 5 (the "XS" variant): Xception extractor (models/xception.py) + TimeSformer over 2048-channel features."""
    from .xception import xception
    cfg = arch.default_tsf_config(2048, num_frames)
    xc = xception(num_classes=1, pretrain_path=None)
    xc.load_state_dict(synth.xception_state(seed))
    tsf = SizeInvariantTimeSformer(config=cfg, require_attention=require_attention)
    tsf.load_state_dict(synth.tsf_state(cfg, seed))
    xc.to(device).train()
    tsf.to(device).train()
    return cfg, xc, tsf


def make_optimizer(cfg, ef, tsf):
    """train.py:180-190: optimizer over chain(extractor, model) parameters; SGD(lr, weight_decay) from the YAML."""
    t = cfg["training"]
    params = list(ef.parameters()) + list(tsf.parameters())
    kind = str(t.get("optimizer", "sgd")).lower()
    fused = {"sgd": optim.FusedSGD, "adamw": optim.FusedAdamW, "adam": optim.FusedAdam}
    plain = {"sgd": torch.optim.SGD, "adamw": torch.optim.AdamW, "adam": torch.optim.Adam}
    if kind not in fused:
        raise ValueError("Error: Invalid optimizer specified in the config file.")      # train.py:191-193
    # one multi-tensor launch per step instead of torch's foreach kernels (same update rule)
    return (fused if params[0].is_cuda else plain)[kind](params, lr=t["lr"], weight_decay=t["weight-decay"])


def build_baseline(num_frames=16, seed=0, device="cuda", extractor=0, drop_connect_rate=arch.DROP_CONNECT_RATE, train_extractor=True):
    """`--model 0` (train.py:120-138, config/baseline.yaml): extractor 0 = EfficientNet-B0 (dim 1280), 1 = Xception (dim 2048), then
    the Baseline head.  Returns (config, extractor, model)."""
    if extractor == 0:
        ex = EfficientNet.from_name("efficientnet-b0", drop_connect_rate=drop_connect_rate)
        ex.load_state_dict(synth.effnet_b0_state(seed))
        dim = 1280
    else:
        from .xception import xception
        ex = xception(num_classes=1, pretrain_path=None)
        ex.load_state_dict(synth.xception_state(seed))
        dim = 2048
    cfg = arch.default_baseline_config(dim, num_frames)
    model = Baseline(config=cfg)
    model.load_state_dict(synth.baseline_state(cfg, seed))
    ex.to(device).train(train_extractor)
    model.to(device).train()
    return cfg, ex, model


def device_batch(batch, num_frames=8, num_identities=2, seed=0, device="cuda", ragged=False, as_uint8=False):
    """Synthetic clips resident on the device: videos are generated there (uint8-valued fp32, BGR 0..255; the reference's
    dataset hands over fp32, deepfakes_dataset.py:339 -- `as_uint8` keeps the raw bytes, which the stems also accept)."""
    aux = synth.clip_inputs(batch, num_frames, num_identities, seed, ragged=ragged, with_video=False)
    g = torch.Generator(device=device).manual_seed(1000 + seed)
    videos = torch.randint(0, 256, (batch, num_frames, 224, 224, 3), generator=g, device=device, dtype=torch.uint8)
    if ragged:
        videos = videos * aux["mask"].to(device)[:, :, None, None, None].to(torch.uint8)
    if not as_uint8:
        videos = videos.float()
    return dict(videos=videos, mask=aux["mask"].to(device), identities_mask=aux["identities_mask"].to(device),
                size_embedding=aux["size_embedding"], positions=aux["positions"].to(device),
                labels=aux["labels"].to(device))


def forward(ef, tsf, batch):
    videos = batch["videos"]
    b, f, h, w, c = videos.shape
    x = videos.reshape(b * f, h, w, c).permute(0, 3, 1, 2)                    # train.py:341 (a view)
    features = ef(x)                                                           # train.py:348
    features = features.reshape(b, f, *features.shape[1:])                    # train.py:354 (a view)
    return tsf(features, mask=batch["mask"], size_embedding=batch["size_embedding"],
               identities_mask=batch["identities_mask"], positions=batch["positions"])   # train.py:355


def _update_metrics(metrics, y_pred, batch_or_labels, loss):
    """train.py:369-374 / test.py:270-277 on the device: `metrics` is a metrics.EpochMetrics."""
    if isinstance(batch_or_labels, dict):
        labels = batch_or_labels["labels"]
        mc = batch_or_labels.get("multiclass_labels") if metrics.multiclass else None
    else:
        labels, mc = batch_or_labels, None
    metrics.update(y_pred, labels, loss, mc)


def _eval_metrics(metrics, out, batch_or_labels):
    """test.py:269-277: the eval loss (plain BCE-with-logits) and the counters, for an eval step that was given `metrics`."""
    y_pred = out[0] if isinstance(out, tuple) else out
    labels = batch_or_labels["labels"] if isinstance(batch_or_labels, dict) else batch_or_labels
    _update_metrics(metrics, y_pred, batch_or_labels, optim.bce_with_logits(y_pred, labels))


def train_step(ef, tsf, optimizer, batch, reducer=None, pos_weight=None, *, metrics=None):
    """One optimisation step (train.py:367-378).  The loss stays on the device (the reference moves the logits to the
    CPU first, one D2H sync per step, train.py:367).  metrics: a metrics.EpochMetrics that takes the step's counters and loss
    (train.py:369-374) in one more launch, without a host read; None = nothing is added to the step."""
    y_pred = forward(ef, tsf, batch)
    if isinstance(y_pred, tuple):
        y_pred = y_pred[0]
    loss = optim.bce_with_logits(y_pred, batch["labels"], pos_weight)          # value + gradient in one launch, on the device
    if metrics is not None:
        _update_metrics(metrics, y_pred, batch, loss)
    optimizer.zero_grad(set_to_none=True)
    loss.backward()
    if reducer is not None:
        reducer.allreduce()
    optimizer.step()
    return loss


@torch.no_grad()
def eval_step(ef, tsf, batch, *, metrics=None):
    """test.py:235-247 / predict.py:401-406: eval forward; returns logits (and attentions if the model was built with them).
    metrics: a metrics.EpochMetrics; the step then also computes the loss against batch["labels"] and updates it (test.py:269-277)."""
    out = forward(ef, tsf, batch)
    if metrics is not None:
        _eval_metrics(metrics, out, batch)
    return out


def baseline_forward(ex, model, batch, freeze_backbone=False):
    """train.py:341-352 with `--model 0`: per-crop logits of the Baseline head, averaged over the clip's frames."""
    videos = batch["videos"]
    b, f, h, w, c = videos.shape
    x = videos.reshape(b * f, h, w, c).permute(0, 3, 1, 2)                    # train.py:341 (a view)
    if freeze_backbone:                                                        # train.py:344-346
        with torch.no_grad():
            features = ex(x)
    else:
        features = ex(x)                                                       # train.py:348
    y_pred = model(features)                                                   # train.py:351
    return torch.mean(y_pred.reshape(-1, f), 1).unsqueeze(1)                   # train.py:352 (num-frames = f)


def baseline_train_step(ex, model, optimizer, batch, pos_weight=None, freeze_backbone=False, *, metrics=None):
    """One `--model 0` optimisation step (train.py:341-378); the optimizer comes from make_optimizer(cfg, ex, model).
    metrics: as in train_step."""
    y_pred = baseline_forward(ex, model, batch, freeze_backbone)
    loss = optim.bce_with_logits(y_pred, batch["labels"], pos_weight)
    if metrics is not None:
        _update_metrics(metrics, y_pred, batch, loss)
    optimizer.zero_grad(set_to_none=True)
    loss.backward()
    optimizer.step()
    return loss


@torch.no_grad()
def baseline_eval_step(ex, model, batch, *, metrics=None):
    """test.py:235-244 with `--model 0`: eval forward, frame-averaged logits [B, 1].  metrics: as in eval_step."""
    out = baseline_forward(ex, model, batch)
    if metrics is not None:
        _eval_metrics(metrics, out, batch)
    return out


def input_gradient(ex, model, batch, pos_weight=None):
    """Gradient of the callers' loss with respect to the face crops: what saliency maps and FGSM / PGD perturbations are made of.
    ex: EfficientNet-B0 or Xception; model: SizeInvariantTimeSformer (forward() above) or Baseline (baseline_forward()); a SlowFast
    model goes to slowfast_input_gradient (ex is not used, pass None).
    Returns (logits, loss, dvideos) with dvideos.shape == batch["videos"].shape, fp32; nothing is added to any parameter's .grad.
    The modules run in the mode they are in (the saliency setting is eval() with every parameter requires_grad_(False); parameters
    that do require grad only cost their weight-gradient launches, and a train-mode extractor updates its BatchNorm running statistics
    as any forward does).  The extractor runs its eager launch sequence: recorded launch plans are neither used nor made.
    uint8 crops have no gradient: cast them first (`videos.float()`)."""
    if isinstance(model, _slowfast.SlowFast):                                  # `--model 2` has no extractor: ex is ignored
        return slowfast_input_gradient(model, batch["videos"], batch["labels"], pos_weight)
    videos = batch["videos"]
    if not torch.is_tensor(videos) or not videos.is_floating_point():
        raise ValueError(f"input_gradient: videos must be a floating-point tensor (got {getattr(videos, 'dtype', type(videos))}); "
                         "cast uint8 crops with .float() first")
    if not videos.is_cuda:
        raise ValueError("input_gradient: videos must be on the device (the extractors have no CPU path)")
    if not isinstance(model, (SizeInvariantTimeSformer, Baseline)):
        raise TypeError(f"input_gradient: model must be a SizeInvariantTimeSformer, a Baseline or a SlowFast, got {type(model).__name__}")
    x = videos.detach().requires_grad_(True)
    local = dict(batch, videos=x)
    with torch.enable_grad():
        y_pred = baseline_forward(ex, model, local) if isinstance(model, Baseline) else forward(ex, model, local)
        logits = y_pred[0] if isinstance(y_pred, tuple) else y_pred
        loss = optim.bce_with_logits(logits, batch["labels"], pos_weight)
        dvideos, = torch.autograd.grad(loss, x)
    return logits.detach(), loss.detach(), dvideos


def build_slowfast(seed=0, device="cuda", head_pool_kernel_sizes=((8, 7, 7), (32, 7, 7)), num_classes=1):
    """`--model 2` (train.py:143-147): slowfast_r50 with blocks[6].proj = nn.Linear(2304, num_classes), on the device, train mode.
    Returns (model, optimizer): SGD(lr, weight_decay) of config/slowfast.yaml through optim.FusedSGD."""
    torch.manual_seed(seed)
    model = _slowfast.slowfast_r50(pretrained=False, head_pool_kernel_sizes=head_pool_kernel_sizes)
    model.blocks[6].proj = torch.nn.Linear(2304, num_classes)
    model.to(device).train()
    opt = (optim.FusedSGD if str(device).startswith("cuda") else torch.optim.SGD)(model.parameters(), lr=0.001, weight_decay=0.0001)
    return model, opt


def slowfast_train_step(model, optimizer, videos, labels, pos_weight=None, *, metrics=None, **transform):
    """One `--model 2` optimisation step (train.py:356-378): input transform, forward, BCE-with-logits, SGD.  videos [B, F, H, W, 3]
    (uint8 or fp32), labels [B]; `transform` goes to slowfast_input_transform (crop_size, side_size, num_frames, interpolation).
    metrics: as in train_step."""
    x = _slowfast.slowfast_input_transform(videos, **transform)
    y_pred = model(x)
    loss = optim.bce_with_logits(y_pred, labels, pos_weight)
    if metrics is not None:
        _update_metrics(metrics, y_pred, labels, loss)
    optimizer.zero_grad(set_to_none=True)
    loss.backward()
    optimizer.step()
    return loss


@torch.no_grad()
def slowfast_eval_step(model, videos, *, metrics=None, labels=None, **transform):
    """test.py:255-259 with `--model 2`: transform (`transform` goes to slowfast_input_transform) and eval forward; returns the logits.
    metrics: a metrics.EpochMetrics, updated with the logits, `labels` [B] (then required) and the eval loss (test.py:269-277)."""
    out = model(_slowfast.slowfast_input_transform(videos, **transform))
    if metrics is not None:
        if labels is None:
            raise ValueError("slowfast_eval_step: metrics needs labels")
        _eval_metrics(metrics, out, labels)
    return out


def slowfast_input_gradient(model, videos, labels, pos_weight=None, **transform):
    """Gradient of the `--model 2` loss with respect to the clips: videos [B, F, H, W, 3] or [B, 3, F, H, W], floating point, on the
    device; `transform` goes to slowfast_input_transform (crop_size, side_size, num_frames, interpolation).  Returns (logits, loss,
    dvideos) with dvideos.shape == videos.shape, fp32: frames the subsampling selected several times (both pathways, repeats of a short
    clip) hold the sum, frames it skipped and pixels outside a centre crop's footprint hold 0.  Nothing is added to any
    parameter's .grad; the model runs in the mode it is in (the saliency setting is eval() with every parameter requires_grad_(False)).
    uint8 clips have no gradient: cast them first."""
    if not torch.is_tensor(videos) or not videos.is_floating_point():
        raise ValueError(f"slowfast_input_gradient: videos must be a floating-point tensor (got {getattr(videos, 'dtype', type(videos))}); "
                         "cast uint8 clips with .float() first")
    if not videos.is_cuda:
        raise ValueError("slowfast_input_gradient: videos must be on the device (SlowFast has no CPU path)")
    x = videos.detach().requires_grad_(True)
    with torch.enable_grad():
        logits = model(_slowfast.slowfast_input_transform(x, **transform))
        loss = optim.bce_with_logits(logits, labels, pos_weight)
        dvideos, = torch.autograd.grad(loss, x)
    return logits.detach(), loss.detach(), dvideos.float()


def aggregate_attentions(attentions, heads, num_frames, frames_per_identity, scale_factor=50000):
    """Reference utils.py:68-96 on the device: attentions = [space, time] as returned by the model with
    require_attention=True.  Returns (aggregated [space, time, combined] lists of num_frames floats, per-identity sums) with the
    reference's own slicing rule for the identity sums (utils.py:87-94)."""
    from . import lib as L
    space, time_ = attentions
    bh, _, n = space.shape
    out = torch.empty(3, num_frames, dtype=torch.float32, device=space.device)
    L.mt.attn_aggregate(space.contiguous(), time_.contiguous(), out, bh, n, num_frames, float(scale_factor))
    agg = out.cpu().tolist()
    comb = agg[-1]
    identity = []
    for index, frames in enumerate(frames_per_identity):
        if index == 0:
            identity.append(sum(comb[:frames - 1]))
        else:
            identity.append(sum(comb[frames_per_identity[index - 1] - 1:frames - 1]))
    return agg, identity


class GraphedEval:
    """Eval forward captured once into a HIP graph (torch.cuda.CUDAGraph) and replayed: the ~440 kernel launches of
    EfficientNet-B0 + TimeSformer become one graph launch, which removes the per-launch host cost that dominates small-batch
    inference (test.py runs bs = 1).  Inputs are copied into static buffers; outputs are static tensors overwritten by replay."""

    def __init__(self, ef, tsf, example_batch):
        assert not ef.training and not tsf.training, "capture the eval() forward"
        self.ef, self.tsf = ef, tsf
        dev = next(tsf.parameters()).device
        # every input lives in a static device buffer (an H2D copy of the reference's host-side size_embedding is not capturable)
        self.static = {k: (v.to(dev).clone() if torch.is_tensor(v) else v) for k, v in example_batch.items()}
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s), torch.no_grad():
            for _ in range(2):                      # warm-up: loads kernels, sets LDS attributes, fills the allocator
                forward(ef, tsf, self.static)
        torch.cuda.current_stream().wait_stream(s)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph), torch.no_grad():
            self.out = forward(ef, tsf, self.static)

    def __call__(self, batch):
        for k, v in batch.items():
            if torch.is_tensor(v):
                self.static[k].copy_(v, non_blocking=True)
        self.graph.replay()
        return self.out
