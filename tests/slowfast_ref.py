"""fp64 torch-CPU functional restatement of SlowFast R50 (pytorchvideo slowfast_r50 as the state-dict contract of
tests/golden/slowfast_r50_manifest.json describes it): the parity anchor of tests/test_gpu_slowfast.py and the torch-conv3d
yardstick of tools/slowfast_step.py.  Written from torch.nn.functional only; nothing here runs on the HIP path."""
import torch
import torch.nn.functional as F

DEPTHS = (3, 4, 6, 3)
SLOW_KT = (1, 1, 3, 3)
FAST_KT = (3, 3, 3, 3)
STRIDE = (1, 2, 2, 2)


def _bn(x, sd, key, training, relu=True):
    y = F.batch_norm(x, sd[key + ".running_mean"], sd[key + ".running_var"], sd[key + ".weight"], sd[key + ".bias"], training, 0.1, 1e-5)
    return F.relu(y) if relu else y


def _block(x, sd, pre, kt, stride, first, training):
    w = lambda n: sd[f"{pre}.{n}.weight"]  # noqa: E731
    a = _bn(F.conv3d(x, w("branch2.conv_a"), padding=(kt // 2, 0, 0)), sd, pre + ".branch2.norm_a", training)
    b = _bn(F.conv3d(a, w("branch2.conv_b"), stride=(1, stride, stride), padding=(0, 1, 1)), sd, pre + ".branch2.norm_b", training)
    c = _bn(F.conv3d(b, w("branch2.conv_c")), sd, pre + ".branch2.norm_c", training, relu=False)
    if first:
        sc = _bn(F.conv3d(x, w("branch1_conv"), stride=(1, stride, stride)), sd, pre + ".branch1_norm", training, relu=False)
    else:
        sc = x
    return F.relu(c + sc)


def _fusion(xs, xf, sd, pre, training):
    f = F.conv3d(xf, sd[pre + ".conv_fast_to_slow.weight"], stride=(4, 1, 1), padding=(3, 0, 0))
    return torch.cat([xs, _bn(f, sd, pre + ".norm", training)], 1)


def forward(sd, slow, fast, training=False, head_pool_kernel_sizes=((8, 7, 7), (32, 7, 7)), dropout_mult=None, taps=None):
    """slow [B, 3, Ts, H, W], fast [B, 3, Tf, H, W] -> logits [B, k].  sd: parameters and BatchNorm buffers (running statistics are
    updated in place when training).  dropout_mult: keep / (1 - p) multipliers of the pooled [B, 2304, Pt, Ph, Pw] tensor (None: no
    dropout).  taps: optional dict that receives the stage outputs (tests: gradient norms per stage)."""
    xs = F.max_pool3d(_bn(F.conv3d(slow, sd["blocks.0.multipathway_blocks.0.conv.weight"], stride=(1, 2, 2), padding=(0, 3, 3)), sd,
                          "blocks.0.multipathway_blocks.0.norm", training), (1, 3, 3), (1, 2, 2), (0, 1, 1))
    xf = F.max_pool3d(_bn(F.conv3d(fast, sd["blocks.0.multipathway_blocks.1.conv.weight"], stride=(1, 2, 2), padding=(2, 3, 3)), sd,
                          "blocks.0.multipathway_blocks.1.norm", training), (1, 3, 3), (1, 2, 2), (0, 1, 1))
    xs = _fusion(xs, xf, sd, "blocks.0.multipathway_fusion", training)
    for s in range(4):
        for i in range(DEPTHS[s]):
            xs = _block(xs, sd, f"blocks.{s + 1}.multipathway_blocks.0.res_blocks.{i}", SLOW_KT[s], STRIDE[s] if i == 0 else 1, i == 0,
                        training)
            xf = _block(xf, sd, f"blocks.{s + 1}.multipathway_blocks.1.res_blocks.{i}", FAST_KT[s], STRIDE[s] if i == 0 else 1, i == 0,
                        training)
        if taps is not None:
            taps[s] = (xs, xf)
        if s < 3:
            xs = _fusion(xs, xf, sd, f"blocks.{s + 1}.multipathway_fusion", training)
    ps = F.avg_pool3d(xs, head_pool_kernel_sizes[0], stride=1)
    pf = F.avg_pool3d(xf, head_pool_kernel_sizes[1], stride=1)
    x = torch.cat([ps, pf], 1)
    if dropout_mult is not None:
        x = x * dropout_mult
    x = F.linear(x.permute(0, 2, 3, 4, 1), sd["blocks.6.proj.weight"], sd["blocks.6.proj.bias"]).permute(0, 4, 1, 2, 3)
    return F.adaptive_avg_pool3d(x, 1).flatten(1)


def normalize_clip(videos, num_frames=32, alpha=4):
    """utils.py:166-186 at 256 x 256 for videos [B, F, H, W, 3]: returns (slow, fast) [B, 3, T, H, W] in the reference's fp32 arithmetic."""
    v = videos.permute(0, 4, 1, 2, 3)
    idx = torch.linspace(0, v.shape[2] - 1, num_frames).long()
    x = torch.index_select(v, 2, idx).float() / 255.0
    mean = torch.as_tensor([0.45] * 3, dtype=x.dtype)[None, :, None, None, None]
    std = torch.as_tensor([0.225] * 3, dtype=x.dtype)[None, :, None, None, None]
    x = (x - mean) / std
    sidx = torch.linspace(0, x.shape[2] - 1, x.shape[2] // alpha).long()
    return torch.index_select(x, 2, sidx), x
