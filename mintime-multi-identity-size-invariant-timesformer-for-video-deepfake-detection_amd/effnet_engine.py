"""Launch sequences (forward, backward) of EfficientNet-B0 on libmintime_hip.  Plumbing only: device buffers via
torch, raw pointers + current stream into the C ABI, one torch.autograd.Function for the whole extractor."""
import threading

import torch

from . import arch
from . import lib as L
from . import plans
from .lib import _new

SLOTS = 32   # replicated fp64 BatchNorm accumulators (spreads atomic traffic)
STREAM_ROWS = 100000   # 1x1 convs with at least this many rows use the streaming kernels (forward and backward)
# Late stages (14 x 14 and 7 x 7 grids, the head) on plane operands (csrc/effnet_planes.hip, gemm_planes.hpp): expand convolutions
# whose input grid is at most EF_PLANES_EXPAND_HW wide, project convolutions whose output grid is at most EF_PLANES_PROJECT_HW wide
# (tools/lab/ef_planes_lab.py: at 14 x 14 the project convolution's producer pass costs what its GEMM saves).
EF_PLANES_EXPAND_HW, EF_PLANES_PROJECT_HW = 14, 7


def param_list(model):
    ps = [model._conv_stem.weight, model._bn0.weight, model._bn0.bias]
    for blk in model._blocks:
        if blk.spec.has_expand:
            ps += [blk._expand_conv.weight, blk._bn0.weight, blk._bn0.bias]
        ps += [blk._depthwise_conv.weight, blk._bn1.weight, blk._bn1.bias, blk._se_reduce.weight, blk._se_reduce.bias,
               blk._se_expand.weight, blk._se_expand.bias, blk._project_conv.weight, blk._bn2.weight, blk._bn2.bias]
    ps += [model._conv_head.weight, model._bn1.weight, model._bn1.bias]
    return ps


class _BNCtx:
    """Per-BatchNorm scratch: accumulators + folded affine + saved statistics."""

    def __init__(self, dev, C, training, stats_pool):
        self.C = C
        self.scale, self.shift = _new(dev, C), _new(dev, C)
        self.mean_invstd = _new(dev, 2, C)
        self.stats = stats_pool.take(C) if training else None
        self.count = 0.0


class _StatsPool:
    """One zero-filled fp64 buffer per forward, carved into [SLOTS][2][C] accumulators.  Deterministic mode (det=True): each
    accumulator is two 64-bit integer limbs (csrc/common.hpp stat_add: integer atomics add up the same whatever the order the
    blocks arrive in), [2 limbs][SLOTS][2][C], and the kernels are handed `-SLOTS`."""

    def __init__(self, dev, total_channels, det=False):
        self.limbs = 2 if det else 1
        self.buf = L.zeros(total_channels * 2 * SLOTS * self.limbs, torch.float64, dev)
        self.off = 0

    def take(self, C):
        n = 2 * SLOTS * C * self.limbs
        v = self.buf[self.off:self.off + n]
        self.off += n
        return v


def _finalize(bn_mod, ctx, count, training, gamma, beta, slots=SLOTS, st=None):
    """slots < 0 (deterministic mode): the producers' statistics are integer limbs (csrc/common.hpp stat_add, _StatsPool).
    st: the stream to launch on (default: the current stream)."""
    ctx.count = float(count)
    L.mt.bn_finalize(ctx.stats, slots, float(count), gamma, beta, bn_mod.running_mean, bn_mod.running_var, ctx.scale, ctx.shift,
                     ctx.mean_invstd, ctx.C, bn_mod.eps, bn_mod.momentum, 1 if training else 0, L.stream_ptr() if st is None else st)
    if training:
        _track(bn_mod.num_batches_tracked)


# num_batches_tracked counters touched by the running forward: bumped by ONE multi-tensor add at its end.  Per thread: forwards of
# different replicas may run concurrently from different Python threads (the reference's nn.DataParallel does that).
_TLS = threading.local()


def _track(counter):
    if not hasattr(_TLS, "tracked"):
        _TLS.tracked = []
    _TLS.tracked.append(counter)


def planes_scope(model, N):
    """(expand-on-planes?, project-on-planes?) per block + head, for a batch of N crops: the plane GEMM wants >= 512 pixel rows."""
    on = L.gemm_split_enabled()
    blocks = model._blocks
    exp = [on and b.spec.has_expand and b.spec.hin <= EF_PLANES_EXPAND_HW and N * b.spec.hin * b.spec.hin >= 512 and b.spec.cin % 4 == 0
           for b in blocks]
    proj = [on and b.spec.hout <= EF_PLANES_PROJECT_HW and N * b.spec.hout * b.spec.hout >= 512 for b in blocks]
    last = blocks[-1].spec
    head = on and last.hout <= EF_PLANES_EXPAND_HW and N * last.hout * last.hout >= 512
    return exp, proj, head


def weight_planes(model, params, exp, proj, head):
    """Plane tensors of the 1x1-conv weights that run on plane operands, re-split from the fp32 weights by ONE launch per forward
    (mt_split_planes_blk_multi; cf. tsf_planes.weight_planes).  Returns ({("e", block) | ("p", block) | "head": planes}, the saved
    serial of their holder or None)."""
    blocks = model._blocks
    sel, pos = [], 3
    for bi, blk in enumerate(blocks):
        if blk.spec.has_expand:
            if exp[bi]:
                sel.append((("e", bi), params[pos], blk.spec.cexp, blk.spec.cin))
            pos += 3
        if proj[bi]:
            sel.append((("p", bi), params[pos + 7], blk.spec.cout, blk.spec.cexp))
        pos += 10
    if head:
        sel.append(("head", params[pos], arch.HEAD_COUT, arch.HEAD_CIN))
    if not sel:
        return {}, None
    # one cache entry per (weight storage, selection): another batch size selects other convolutions, and a recorded launch plan
    # (plans.py) keeps reading the table and the plane tensors of the entry it was recorded with
    ident = tuple((k, w.data_ptr()) for k, w, _, _ in sel)
    caches = model.__dict__.setdefault("_ef_wplanes_cache", {})
    if len(caches) > 4 and ident not in caches:
        caches.pop(next(iter(caches)))
    cache = caches.get(ident)
    if cache is None:
        holder, rows, first = {}, [], 0
        dev = sel[0][1].device
        for key, w, r, c in sel:
            if w.dtype != torch.float32 or not w.is_contiguous() or w.numel() != r * c:
                raise L.MintimeHipError("plane path needs contiguous fp32 1x1-conv weights")
            t = L.planes_empty(r, c, dev)
            holder[key] = t
            rows.append((w.data_ptr(), t.data_ptr(), r, c, first))
            first += t.shape[1] * t.shape[2]
        host = torch.tensor(rows, dtype=torch.int64).pin_memory()
        cache = caches[ident] = dict(holder=holder, host=host, table=host.to(dev, non_blocking=True), blocks=first, count=len(rows),
                                     serial=plans.PlaneSerial("the 1x1-conv weights"))
    L.mt.split_planes_blk_multi(cache["table"], cache["count"], cache["blocks"])       # (a plan being recorded pins the table)
    return cache["holder"], cache["serial"].touch([w for _, w, _, _ in sel])


def _bump_tracked(plan=None):
    tracked = getattr(_TLS, "tracked", None)
    if tracked:
        if plan is not None:
            plan.extra["tracked"] = list(tracked)       # a replayed forward bumps the same counters (plans.py)
        torch._foreach_add_(tracked, 1)
        tracked.clear()


def _dc_gates(model, N, dev):
    """Per-sample drop-connect gates (utils.py:129-154), train mode only: floor(keep + U[0,1)) / keep, keep = 1 - rate*idx/16
    (model.py:280-282).  ONE draw for all gated blocks (rows in block order); `model.drop_connect_uniform`, when set, supplies
    the uniforms instead of torch.rand (callable (n_rows, N, device) -> [n_rows, N]; parity tests feed the oracle's draws).
    Returns (gated block indices, gates [n_gated, N]) or ([], None)."""
    blocks = model._blocks
    if not (model.training and model.drop_connect_rate > 0):
        return [], None
    gated = [bi for bi, blk in enumerate(blocks) if blk.spec.skip and model.drop_connect_rate * float(bi) / len(blocks) > 0]
    if not gated:
        return [], None
    sampler = getattr(model, "drop_connect_uniform", None)
    u = sampler(len(gated), N, dev) if sampler is not None else torch.rand(len(gated), N, device=dev, dtype=torch.float32)
    cache = model.__dict__.setdefault("_dc_keep_cache", {})
    key = (str(dev), model.drop_connect_rate)
    if key not in cache:    # uploaded once, not per step
        cache[key] = torch.tensor([1.0 - model.drop_connect_rate * float(bi) / len(blocks) for bi in gated],
                                  dtype=torch.float32, device=dev).unsqueeze(1)
    keep = cache[key]
    return gated, torch.floor(keep + u.to(device=dev, dtype=torch.float32)) / keep


def effnet_forward(model, x_nhwc, params, training, save, want_blocks=False, plan=None):
    """x_nhwc [N,H,W,3] contiguous fp32.  Returns (feat [N*Ho*Wo, 1280], saved or None, block outputs or None).
    plan: the plans.NetPlan being recorded (it keeps the gate buffer and the tracked counters for its replays)."""
    lib = L.get()
    dev = x_nhwc.device
    N, H, W, _ = x_nhwc.shape
    # every block's row count below comes from the model's specs (arch.effnet_b0_blocks(image_size): one hin / hout per block), so the
    # walk serves square crops of the model's image_size and nothing else: any other shape would read past the stem's output.  Refused
    # here, before anything is allocated or launched
    if H != model.image_size or W != model.image_size:
        raise ValueError(f"EfficientNet engine: crops of H = {H} by W = {W}, the model was built for "
                         f"{model.image_size} x {model.image_size} (one size per axis in every MBConv spec)")
    # the stem's leading TF-SAME pad (utils.py:248-276: the smaller half of the total goes in front): 0 for an even size, 1 for an odd
    Hc, Wc = (H + 1) // 2, (W + 1) // 2
    stem_pad = max((Hc - 1) * 2 + 3 - H, 0) // 2
    blocks = model._blocks
    total_c = arch.STEM_COUT + arch.HEAD_COUT + sum((b.spec.cexp if b.spec.has_expand else 0) + b.spec.cexp + b.spec.cout
                                                    for b in blocks)
    det = training and L.deterministic()          # MT_DETERMINISTIC: the producers' statistics as integer limbs (order-independent)
    pool = _StatsPool(dev, total_c, det) if training else None
    it = iter(params)
    slots = -SLOTS if det else SLOTS
    epi = L.EPI_STATS if training else L.EPI_STORE
    saved = {"blocks": []} if save else None
    pl_exp, pl_proj, pl_head = planes_scope(model, N)
    wpl, w_serial = weight_planes(model, params, pl_exp, pl_proj, pl_head)
    y_p = None                   # planes of the current block input y (written by the producing block's bn_act when the next conv wants them)

    # ---- stem
    w_stem, g0, b0 = next(it), next(it), next(it)
    bn = _BNCtx(dev, arch.STEM_COUT, training, pool)
    z = _new(dev, N * Hc * Wc, arch.STEM_COUT)
    # stem: streaming MFMA kernel (stem_fwd.hip; uint8 crops converted on the fly, BatchNorm statistics in the same pass).  The
    # im2col-prologue GEMM it replaced (K = 27 taps padded to 28) stays the path for crops wider than the kernel's LDS row tile.
    if W <= 512:
        L.mt.stem_conv_fwd(x_nhwc, 1 if x_nhwc.dtype == torch.uint8 else 0, w_stem, z, bn.stats, slots, N, H, W)
    else:
        wp = _new(dev, arch.STEM_COUT, 28)
        L.mt.conv_weight_pack(w_stem, wp, arch.STEM_COUT, 3, 3, 28, 0)
        L.gemm(L.OP_NT, x_nhwc, wp, z, N * Hc * Wc, arch.STEM_COUT, 28, 28, 28, arch.STEM_COUT, prologue=L.PRO_IM2COL, epilogue=epi,
               stats=bn.stats, stats_slots=slots, conv=(H, W, 3, Hc, Wc, 3, 2, stem_pad, 0, 1 if x_nhwc.dtype == torch.uint8 else 0))
    _finalize(model._bn0, bn, N * Hc * Wc, training, g0, b0, slots)
    if save:
        saved["stem"] = dict(x=x_nhwc, z=z, bn=bn)
    cur_z, cur_bn = z, bn        # "virtual" activated tensor: swish(bn(z))
    y = None                     # materialised block output (narrow tensor)
    ys = [] if want_blocks else None

    gated, gates = _dc_gates(model, N, dev) if training else ([], None)
    dc_gates = {bi: gates[j] for j, bi in enumerate(gated)}
    if plan is not None:
        plan.extra["gates"] = gates
    for bi, blk in enumerate(blocks):
        s = blk.spec
        M_in = N * s.hin * s.hin
        M_out = N * s.hout * s.hout
        rec = {"spec": s}
        if s.has_expand:
            w_e, g, b = next(it), next(it), next(it)
            bn_e = _BNCtx(dev, s.cexp, training, pool)
            z_e = _new(dev, M_in, s.cexp)
            if pl_exp[bi]:
                # late stages: y arrives as planes (written by the block above), the weight planes were split at the top
                L.gemm_planes(L.OP_NT, y_p, wpl[("e", bi)], M_in, s.cexp, s.cin, Cout=z_e, ldc=s.cexp, epilogue=epi, stats=bn_e.stats,
                              stats_slots=slots)
                rec.update(y_p=y_p, we_p=wpl[("e", bi)])
            elif M_in >= STREAM_ROWS and lib.mt_conv1x1_rows_supported(s.cin, s.cexp, 0):   # few channels, very many rows: streaming kernel
                L.mt.conv1x1_rows(y, None, w_e, s.cin, 0, None, None, None, 1, 0, None, z_e, bn_e.stats, slots, M_in, s.cin, s.cexp)
            else:
                L.gemm(L.OP_NT, y, w_e, z_e, M_in, s.cexp, s.cin, s.cin, s.cin, s.cexp, epilogue=epi, stats=bn_e.stats, stats_slots=slots)
            _finalize(blk._bn0, bn_e, M_in, training, g, b, slots)
            rec.update(z_e=z_e, bn_e=bn_e)
            dw_in, dw_bn = z_e, bn_e
        else:
            dw_in, dw_bn = cur_z, cur_bn
        w_d, g, b = next(it), next(it), next(it)
        bn_d = _BNCtx(dev, s.cexp, training, pool)
        z_d = _new(dev, M_out, s.cexp)
        L.mt.dwconv_fwd(dw_in, dw_bn.scale, dw_bn.shift, w_d, z_d, bn_d.stats, slots, N, s.hin, s.hin, s.cexp, s.k, s.s, 1)
        _finalize(blk._bn1, bn_d, M_out, training, g, b, slots)
        w_r, b_r, w_x, b_x = next(it), next(it), next(it), next(it)
        pooled, gate = _new(dev, N, s.cexp), _new(dev, N, s.cexp)
        hidden = _new(dev, N, s.cse)          # squeeze pre-activations: the gate kernel reads them (and backward keeps them)
        hw = s.hout * s.hout
        parts = lib.mt_se_pool_parts(N, hw, s.cexp)
        partial = _new(dev, N, parts, s.cexp)
        L.mt.se_pool_fwd(z_d, bn_d.scale, bn_d.shift, partial, N, hw, s.cexp, parts)
        L.mt.se_gate_fwd(partial, parts, w_r, b_r, w_x, b_x, pooled, gate, hidden, N, s.cexp, s.cse)
        w_p, g, b = next(it), next(it), next(it)
        bn_p = _BNCtx(dev, s.cout, training, pool)
        z_p = _new(dev, M_out, s.cout)
        if pl_proj[bi]:
            # 7 x 7 stage: the operand swish(bn1(z_d)) * gate written once as planes (kept for the weight gradient), the GEMM only DMAs
            a_p = L.planes_empty(M_out, s.cexp, dev)
            L.mt.bn_swish_gate_planes(z_d, bn_d.scale, bn_d.shift, gate, hw, a_p, M_out, s.cexp)
            L.gemm_planes(L.OP_NT, a_p, wpl[("p", bi)], M_out, s.cout, s.cexp, Cout=z_p, ldc=s.cout, epilogue=epi, stats=bn_p.stats,
                          stats_slots=slots)
            rec.update(a_p=a_p, wp_p=wpl[("p", bi)])
        elif M_out >= STREAM_ROWS and lib.mt_conv1x1_rows_supported(s.cexp, s.cout, 1):
            L.mt.conv1x1_rows(z_d, None, w_p, s.cexp, 0, bn_d.scale, bn_d.shift, gate, hw, 1, None, z_p, bn_p.stats, slots, M_out, s.cexp,
                              s.cout)
        else:
            L.gemm(L.OP_NT, z_d, w_p, z_p, M_out, s.cout, s.cexp, s.cexp, s.cexp, s.cout, prologue=L.PRO_BN_SWISH_GATE, epilogue=epi,
                   scale=bn_d.scale, shift=bn_d.shift, gate=gate, hw=hw, stats=bn_p.stats, stats_slots=slots)
        _finalize(blk._bn2, bn_p, M_out, training, g, b, slots)
        # block output: bn2(z_p) [* drop-connect gate] [+ block input]
        dc = dc_gates.get(bi)
        y_new = _new(dev, M_out, s.cout)
        next_planes = pl_exp[bi + 1] if bi + 1 < len(blocks) else pl_head
        if next_planes:
            y_p = L.planes_empty(M_out, s.cout, dev)
            L.mt.bn_act_fwd_planes(z_p, bn_p.scale, bn_p.shift, y if s.skip else None, y_new, M_out, s.cout, 0, dc, hw, y_p)
        else:
            y_p = None
            L.mt.bn_act_fwd(z_p, bn_p.scale, bn_p.shift, y if s.skip else None, y_new, M_out, s.cout, 0, dc, hw)
        if save:
            rec.update(y_in=y, dw_in=dw_in, dw_bn=dw_bn, z_d=z_d, bn_d=bn_d, pooled=pooled, hidden=hidden, gate=gate, z_p=z_p,
                       bn_p=bn_p, dc=dc)
            saved["blocks"].append(rec)
        y = y_new
        if want_blocks:
            ys.append(y.view(N, s.hout, s.hout, s.cout).permute(0, 3, 1, 2))

    # ---- head
    w_h, g, b = next(it), next(it), next(it)
    s = blocks[-1].spec
    M = N * s.hout * s.hout
    bn_h = _BNCtx(dev, arch.HEAD_COUT, training, pool)
    z_h = _new(dev, M, arch.HEAD_COUT)
    if pl_head:
        L.gemm_planes(L.OP_NT, y_p, wpl["head"], M, arch.HEAD_COUT, arch.HEAD_CIN, Cout=z_h, ldc=arch.HEAD_COUT, epilogue=epi,
                      stats=bn_h.stats, stats_slots=slots)
    else:
        L.gemm(L.OP_NT, y, w_h, z_h, M, arch.HEAD_COUT, arch.HEAD_CIN, arch.HEAD_CIN, arch.HEAD_CIN, arch.HEAD_COUT, epilogue=epi,
               stats=bn_h.stats, stats_slots=slots)
    _finalize(model._bn1, bn_h, M, training, g, b, slots)
    feat = _new(dev, M, arch.HEAD_COUT)
    L.mt.bn_act_fwd(z_h, bn_h.scale, bn_h.shift, None, feat, M, arch.HEAD_COUT, 1, None, 1)
    if save:
        saved["head"] = dict(y_in=y, z=z_h, bn=bn_h, y_p=y_p if pl_head else None, w_p=wpl.get("head"))
        saved["w_serial"] = w_serial
    _bump_tracked(plan)
    return feat, saved, ys


class _EffNetFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, want_blocks, x_nhwc, *params):
        want_blocks, grad_on = want_blocks
        save = grad_on and any(ctx.needs_input_grad)      # see tsf_engine._TSFFunction.forward
        N, H, W, _ = x_nhwc.shape
        ctx.shape = (N, H, W)
        ctx.model, ctx.params, ctx.training = model, params, model.training
        stream = key = state = None
        # (crops that require grad -- saliency, adversarial examples -- run the eager launch sequence: plan keys do not carry them)
        if save and not want_blocks and not ctx.needs_input_grad[2]:
            stream = torch.cuda.current_stream(x_nhwc.device).cuda_stream
            state = list(params) + list(model.buffers())       # (what a recording holds the addresses of)
            key = ("ef", tuple(x_nhwc.shape), x_nhwc.dtype, model.training, L.deterministic(), L.gemm_split_enabled(),
                   float(model.drop_connect_rate), tuple(ctx.needs_input_grad[3:]), stream,
                   float(model._bn0.momentum), float(model._bn0.eps))       # (scalars a recorded call holds by value)

        def body(ins, plan):
            feat, saved, ys = effnet_forward(model, ins["x"], params, model.training, save, want_blocks, plan=plan)
            for t in ys or ():
                ctx.mark_non_differentiable(t)
            return (feat, *(ys or ())), saved

        def gates(np_):      # this step's drop-connect draws into the recorded gate buffer
            if np_.extra.get("gates") is not None:
                np_.extra["gates"].copy_(_dc_gates(model, N, x_nhwc.device)[1])
        return plans.forward(ctx, model, key, stream, state, {"x": x_nhwc}, body, before_run=gates)

    @staticmethod
    def backward(ctx, dfeat, *unused):
        from .effnet_backward import effnet_backward, LAST_RUN
        need_dx, need_dp = ctx.needs_input_grad[2], ctx.needs_input_grad[3:]

        def body(g, keep_saved, plan):
            dx, dparams = effnet_backward(ctx.model, ctx.params, ctx.saved, ctx.shape, ctx.training, g, need_dx, need_dp,
                                          keep_saved=keep_saved, plan=plan)
            return (dx,), dparams
        return (None, None) + plans.backward(ctx, "EfficientNet", dfeat.contiguous(), body,
                                             after_run=lambda np_: LAST_RUN.update(np_.extra["last_run"]))


def effnet_apply(model, inputs, want_blocks=False):
    if not inputs.is_cuda:
        raise L.MintimeHipError("EfficientNet (MI355X build) needs device tensors; there is no CPU path")
    if inputs.dim() != 4 or inputs.shape[1] != 3:
        raise ValueError(f"expected [N,3,H,W] input, got {tuple(inputs.shape)}")
    if inputs.shape[2] != model.image_size or inputs.shape[3] != model.image_size:
        raise ValueError(f"static TF-SAME padding was built for {model.image_size}x{model.image_size} inputs "
                         f"(utils.py:248-276); got {tuple(inputs.shape[2:])}")
    # logical NCHW, physical NHWC: a view when the caller did `rearrange(videos, 'b f h w c -> (b f) c h w')` (train.py:341).
    # uint8 crops (what cv2 produces before deepfakes_dataset.py:339 casts them to float) are ingested as they are: the stem's
    # gather converts on the fly, which cuts the H2D copy and the stem's input traffic 4x (next-row f2).
    x_nhwc = (inputs if inputs.dtype == torch.uint8 else inputs.float()).permute(0, 2, 3, 1)
    if not x_nhwc.is_contiguous():
        x_nhwc = x_nhwc.contiguous()
    outs = _EffNetFunction.apply(model, (want_blocks, torch.is_grad_enabled()), x_nhwc, *param_list(model))
    feat = outs[0]
    n = inputs.shape[0]
    ho = model._blocks[-1].spec.hout
    feat_nchw = feat.view(n, ho, ho, arch.HEAD_COUT).permute(0, 3, 1, 2)     # NHWC-strided [N,1280,7,7]
    return feat_nchw, list(outs[1:])
