"""Baseline model (reference models/baseline.py:15-37, `--model 0` of train.py / test.py) on libmintime_hip (MI355X).

Python surface of the reference: `Baseline(config)` reads `dim`, `mlp-dim` and `num-classes`; `forward(x[N, dim, H, W], mask=None)`
returns `[N, num-classes]` logits (mask is ignored, as in the reference); the state-dict keys and shapes are the reference's
(`mlp_head.0.weight [mlp, dim]`, `mlp_head.0.bias`, `mlp_head.1.weight [k, mlp]`, `mlp_head.1.bias`).

Every MINTIME configuration has num-classes 1 and nothing between the two Linears, so AdaptiveAvgPool2d(1) -> Linear -> Linear is the
rank-1 map logit_i = mean_p(x_i[p, :]) . v + c0 with v = W1^T w2 and c0 = w2 . b1 + b2 (include/mintime_hip.h, "Baseline head").  The
features are read once, in the layout the extractors hand over (an NHWC buffer seen through a permute) or NCHW-contiguous.
"""
import math

import torch
from torch import nn

from . import lib as L
from . import plans
from .timesformer import _Linear, _Seq

# what the last backward launched (tests: frozen parameters and an input without gradient cost nothing)
LAST_RUN = {"param_grads": None, "dfeat": None}


class Baseline(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.dim = config["model"]["dim"]
        self.mlp_dim = config["model"]["mlp-dim"]
        self.num_classes = config["model"]["num-classes"]
        if self.num_classes != 1:
            raise NotImplementedError(f"Baseline: the HIP head is the rank-1 form of a num-classes 1 head (W1^T w2); got num-classes "
                                      f"{self.num_classes} (every MINTIME config and the callers' BCE use 1)")
        self.mlp_head = _Seq({0: _Linear(self.dim, self.mlp_dim), 1: _Linear(self.mlp_dim, self.num_classes)})
        self.reset_parameters()

    def reset_parameters(self):
        """nn.Linear's default initialisation (reference baseline.py:26-29 builds plain nn.Linear layers)."""
        for lin in (getattr(self.mlp_head, "0"), getattr(self.mlp_head, "1")):
            nn.init.kaiming_uniform_(lin.weight, a=math.sqrt(5))
            bound = 1.0 / math.sqrt(lin.weight.shape[1])
            nn.init.uniform_(lin.bias, -bound, bound)

    def _param_list(self):
        l0, l1 = getattr(self.mlp_head, "0"), getattr(self.mlp_head, "1")
        return [l0.weight, l0.bias, l1.weight, l1.bias]

    def forward(self, x, mask=None):
        return baseline_apply(self, x)


class _BaselineHeadFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, mode, x, w1, b1, w2, b2):
        grad_on, layout = mode                                 # layout 0: x is [n, H, W, C]; 1: [n, C, H, W] (contiguous)
        n = x.shape[0]
        C, m = model.dim, model.mlp_dim
        hw = x.shape[1] * x.shape[2] if layout == 0 else x.shape[2] * x.shape[3]
        save = grad_on and any(ctx.needs_input_grad)           # see tsf_engine._TSFFunction.forward
        dev = x.device
        vc = torch.empty(C + 1, dtype=torch.float32, device=dev)
        pooled = torch.empty(n, C, dtype=torch.float32, device=dev) if save else None
        part = torch.empty(n * ((C + 255) // 256), dtype=torch.float32, device=dev)
        logits = torch.empty(n, 1, dtype=torch.float32, device=dev)
        L.mt.baseline_head_fwd(x, layout, n, hw, C, m, w1, b1, w2, b2, vc, pooled, part, logits)
        ctx.model, ctx.dims, ctx.params, ctx.x_shape = model, (layout, n, hw, C, m), (w1, b1, w2, b2), x.shape
        ctx.saved = dict(pooled=pooled, vc=vc, stamp=plans.stamp((w1, b1, w2, b2))) if save else None
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        if ctx.saved is None:
            plans.refuse_second_pass("Baseline")
        w1, b1, w2, b2 = ctx.params
        plans.check_stamp(ctx.params, ctx.saved["stamp"], "Baseline", "the head weights", "v = W1^T w2 was formed from the old values")
        layout, n, hw, C, m = ctx.dims
        need_x = ctx.needs_input_grad[2]
        need_p = ctx.needs_input_grad[3:7]
        g = dlogits.reshape(-1).contiguous().float()
        dev = g.device
        dw1 = torch.empty(m, C, dtype=torch.float32, device=dev) if need_p[0] else None
        db1 = torch.empty(m, dtype=torch.float32, device=dev) if need_p[1] else None
        dw2 = torch.empty(1, m, dtype=torch.float32, device=dev) if need_p[2] else None
        db2 = torch.empty(1, dtype=torch.float32, device=dev) if need_p[3] else None
        dx = torch.empty(ctx.x_shape, dtype=torch.float32, device=dev) if need_x else None
        work = torch.empty(((n + 31) // 32 + 1) * (C + 4), dtype=torch.float32, device=dev) if any(need_p) else None
        if need_x or any(need_p):
            L.mt.baseline_head_bwd(g, ctx.saved["pooled"], ctx.saved["vc"], n, hw, C, m, w1, b1, w2, dw1, db1, dw2, db2, dx, layout, work)
        LAST_RUN.update(param_grads=any(need_p), dfeat=need_x)
        ctx.saved = None
        return None, None, dx, dw1, db1, dw2, db2


def baseline_apply(model, x):
    if not x.is_cuda:
        raise L.MintimeHipError("Baseline (MI355X build) needs device tensors; there is no CPU path")
    if x.dim() != 4 or x.shape[1] != model.dim:
        raise ValueError(f"expected [N, {model.dim}, H, W] features, got {tuple(x.shape)}")
    params = model._param_list()
    if any(not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous() for p in params):
        raise L.MintimeHipError("Baseline: the head's parameters must be contiguous fp32 device tensors (call .cuda())")
    x = x.float()
    # the extractors hand over an NHWC buffer seen through permute(0, 3, 1, 2): read it as it is, and the input gradient comes back in
    # that layout too (autograd's permute backward then gives the extractor a contiguous [N*H*W, C] buffer, no copy)
    xb, layout = x.permute(0, 2, 3, 1), 0
    if not xb.is_contiguous() or xb.data_ptr() % 16:
        if x.is_contiguous() and x.data_ptr() % 16 == 0:
            xb, layout = x, 1
        else:
            xb = x.contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1)     # one copy
            if xb.data_ptr() % 16:
                xb = xb.clone()
    return _BaselineHeadFunction.apply(model, (torch.is_grad_enabled(), layout), xb, *params)
