"""Launch sequences (forward and backward) of the Size-Invariant TimeSformer on libmintime_hip.

Python here is plumbing only: it allocates device buffers through torch, passes raw pointers + the current
HIP stream to the C ABI, and wires the result into autograd with ONE torch.autograd.Function for the whole
transformer (inputs: token-major features + every parameter; the backward pass is our own reverse launch
sequence, not torch autograd over torch ops).
"""
import os
import types

import torch

from . import arch
from . import lib as L
from . import plans, tsf_planes
from .lib import _new
from .tsf_backward import tsf_backward


def _as_tokens(x):
    """[B,F,C,h,w] (any strides) -> token-major [B*F*h*w, C] contiguous.  Zero-copy when x is the NHWC-strided
    view our EfficientNet returns; otherwise one layout copy (the reference always pays it, :227)."""
    b, f, c, h, w = x.shape
    t = x.permute(0, 1, 3, 4, 2)
    if not t.is_contiguous():
        t = t.contiguous()
    return t.reshape(b * f * h * w, c)


class _Aux:
    """Device-side copies of the per-clip side inputs in the dtypes the kernels read."""

    def __init__(self, model, x, mask, identities_mask, size_embedding, positions):
        dev = x.device
        b, f = x.shape[0], x.shape[1]
        if mask is None:
            mask = torch.ones(b, f, dtype=torch.bool, device=dev)
        if identities_mask is None:
            identities_mask = torch.ones(b, f, f, dtype=torch.bool, device=dev)
        self.mask = mask.to(device=dev, dtype=torch.uint8).contiguous()
        self.ident = identities_mask.to(device=dev, dtype=torch.uint8).contiguous()
        self.sizes = None
        rows = model.pos_emb.weight.shape[0]
        if model.enable_size_emb:
            if size_embedding is not None and not size_embedding.is_cuda and size_embedding.numel():
                # the reference's callers leave it on the host (train.py:355): range-check for free, like nn.Embedding would
                lo, hi = int(size_embedding.min()), int(size_embedding.max())
                if lo < 0 or hi >= model.size_emb.weight.shape[0]:
                    raise IndexError(f"size_embedding values must lie in [0, {model.size_emb.weight.shape[0]}); got [{lo}, {hi}]")
            # arrives as a CPU int32 tensor in the reference call sites (train.py:355); moved here like :245 -- through a pinned
            # staging buffer and an async copy: a pageable H2D copy blocks the host until the stream has drained the whole
            # extractor forward, and the GPU then idles (~0.3 ms per step) while the host re-fills the launch queue
            se = size_embedding.to(dtype=torch.int32)
            if not se.is_cuda:
                se = se.contiguous().pin_memory().to(dev, non_blocking=True)
            self.sizes = se.to(device=dev).contiguous()
        self.positions = None
        if model.enable_pos_emb:
            if not positions.is_cuda and positions.numel():
                lo, hi = int(positions.min()), int(positions.max())
                if lo < 0 or hi >= rows:
                    raise IndexError(f"positions must lie in [0, {rows}); got [{lo}, {hi}]")
            self.positions = positions.to(device=dev, dtype=torch.int64).contiguous()
        # device-resident indices cannot be checked without a sync: the embedding kernels clamp them and raise a sticky flag
        # that is looked at when the NEXT forward starts (a deferred device-side assert, like nn.Embedding on a GPU)
        self.err = _index_flag(model, dev)


def _index_flag(model, dev):
    st = model.__dict__.setdefault("_index_flags", {})
    key = str(dev)
    if key in st:
        flag, host, ev = st[key]
        if ev is not None and not torch.cuda.is_current_stream_capturing() and ev.query():
            bad = int(host[0])
            if bad:
                flag.zero_()
                host.zero_()
                what = " and ".join(n for bit, n in ((1, "positions"), (2, "size_embedding")) if bad & bit)
                raise IndexError(f"an earlier SizeInvariantTimeSformer.forward received out-of-range {what} indices "
                                 "(they were clamped into the embedding tables)")
    else:
        st[key] = [torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32).pin_memory(), None]
    return st[key]


def _publish_index_flag(state):
    if torch.cuda.is_current_stream_capturing():
        return
    flag, host, _ = state
    host.copy_(flag, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    state[2] = ev


def tsf_forward(model, feat, aux, params, B, F, n, save):
    """Runs the forward launch sequence.  Returns (logits, space_att, time_att, saved-dict or None)."""
    dev = feat.device
    D, H, dh, C_in = model.dim, model.heads, model.dim_head, model.channels
    inner = H * dh
    N = 1 + F * n
    M = B * N
    eps = arch.LN_EPS
    scale = float(dh) ** -0.5
    it = iter(params)
    w_pe, b_pe, cls, pos_w, size_w = next(it), next(it), next(it), next(it), next(it)

    x = _new(dev, B, N, D)
    L.gemm(L.OP_NT, feat, w_pe, x, B * F * n, D, C_in, C_in, C_in, D, bias=b_pe, c_map=(F * n, N, 1))
    L.mt.embed_fwd(x, cls, pos_w, size_w, aux.positions, aux.sizes, B, F, n, D, pos_w.shape[0],
                   size_w.shape[0] if size_w is not None else 0, aux.err[0])
    _publish_index_flag(aux.err)

    saved = {"layers": []} if save else None
    if save and M >= 4096 and L.gemm_split_enabled() and not torch.cuda.is_current_stream_capturing():
        # Data gradients contract over a weight's ROW index: with the weight as stored that is a k-major B operand (eight strided
        # dword loads per thread in the split loop); over the transposed weight it is the same k-contiguous NT form as the forward
        # (two float4 loads): -10 % per launch (profiles/r02_gemm_split_lab.txt).  The 36 transposes (48 M floats) run on the
        # weight-gradient stream, which is idle through the forward.
        side = L.SideStream(dev)
        wts = list(params[5:5 + 16 * model.depth])
        sel = [(li, off) for li in range(model.depth) for off in (2, 3, 7, 8, 12, 14)]   # w_qkv, w_o (time); w_qkv, w_o (space); net.0 / net.3
        key = tuple(wts[16 * li + off].data_ptr() for li, off in sel)
        cache = getattr(model, "_wT_cache", None)
        if cache is None or cache["key"] != key:
            # PERSISTENT transposed copies (192 MB at depth 9) and one device table for mt_transpose_multi: no allocation and one
            # launch per step.  (Per-step buffers under the side stream needed record_stream(main), and the caching allocator then
            # queued one event record per buffer on the main queue when they died: 0.3 ms of idle device before the extractor's
            # backward; 54 torch copy kernels cost the host ~2 ms per step.)  Rewritten at the start of every training forward: the
            # side stream waits for everything the main stream has enqueued, i.e. for the previous step's data gradients.
            holder, rows, tiles = {}, [], 0
            for li, off in sel:
                w = wts[16 * li + off]
                if w.dtype != torch.float32 or not w.is_contiguous():
                    raise L.MintimeHipError("transposed-weight cache needs contiguous fp32 Linear weights")
                t = torch.empty(w.shape[1], w.shape[0], dtype=torch.float32, device=dev)
                holder[(li, off)] = t
                rows.append((w.data_ptr(), t.data_ptr(), w.shape[0], w.shape[1], tiles))
                tiles += ((w.shape[0] + 31) // 32) * ((w.shape[1] + 31) // 32)
            host = torch.tensor(rows, dtype=torch.int64).pin_memory()
            cache = dict(key=key, holder=holder, table=host.to(dev, non_blocking=True), host=host, tiles=tiles, count=len(rows))
            model._wT_cache = cache

        def transpose_all():
            L.mt.transpose_multi(cache["table"], cache["count"], cache["tiles"])
        if side.enabled:       # with MT_SIDE_STREAM=0 the transposes would sit on the critical path: the NN form is used instead
            cache["serial"] = cache.get("serial", 0) + 1       # a later forward rewrites the buffers: backward checks this
            saved["wT"], saved["wT_ready"], saved["wT_serial"] = cache["holder"], side.launch(transpose_all, reads=wts), cache["serial"]
    # Optional on this engine (MT_TSF_PRUNE_LAST=1, off by default here; the plane path, tsf_planes.prune_last, has it on by default from 32 clips up):
    # dead-row pruning of the LAST layer.  The classification head reads the cls
    # token only (size_invariant_timesformer.py:270-276), so everything the last layer computes for the 392 patch rows AFTER its
    # time attention is never read: the space attention's patch queries and out-projection rows and the whole feed-forward block
    # (the reference computes them and throws them away; their gradients are exactly zero).  With the switch on those rows are not
    # computed: the cls query attends to all keys as before, out-projection / LayerNorm / FF1 / FF2 run on the B cls rows.  Logits,
    # attentions and every gradient are the same numbers (tests/test_gpu_tsf.py); 7 % of the TimeSformer's FLOPs disappear.
    prune_last = os.environ.get("MT_TSF_PRUNE_LAST", "0") != "0"
    want_att = model.require_attention
    s_att = t_att = None
    xn = _new(dev, M, D)
    qkv = _new(dev, M, 3 * inner)
    o = _new(dev, M, inner)
    hbuf = _new(dev, M, 4 * D)
    for li in range(model.depth):
        last = li == model.depth - 1
        rec = {}
        for mode in (0, 1):   # 0 = time, 1 = space
            g, b_, w_qkv, w_o, b_o = next(it), next(it), next(it), next(it), next(it)
            if save:
                xn, qkv, o = _new(dev, M, D), _new(dev, M, 3 * inner), _new(dev, M, inner)
                stats = _new(dev, M, 2)
            else:
                stats = None
            L.mt.layernorm_fwd(x, g, b_, xn, stats, M, D, eps, None)
            L.gemm(L.OP_NT, xn, w_qkv, qkv, M, 3 * inner, D, D, D, 3 * inner)
            att = None
            if want_att and last:
                att = _new(dev, B * H, 1, N)
                if mode == 0:
                    t_att = att
                else:
                    s_att = att
            if last and mode == 1 and prune_last:
                # cls query only; out-projection + residual on the B cls rows (row stride N: no gather needed)
                L.mt.attn_fwd(qkv, o, att, aux.mask, aux.ident, B, H, F, n, 2, scale, None)
                x_cls = _new(dev, B, D)
                L.gemm(L.OP_NT, o, w_o, x_cls, B, D, inner, N * inner, inner, D, epilogue=L.EPI_BIAS_RES, bias=b_o, R=x, ldr=N * D)
                if save:
                    rec[mode] = dict(x=x, xn=xn, stats=stats, qkv=qkv, o=o)
                x = x_cls
                continue
            L.mt.attn_fwd(qkv, o, att, aux.mask, aux.ident, B, H, F, n, mode, scale, None)
            x_new = _new(dev, B, N, D) if save else x
            L.gemm(L.OP_NT, o, w_o, x_new, M, D, inner, inner, inner, D, epilogue=L.EPI_BIAS_RES, bias=b_o, R=x, ldr=D)
            if save:
                rec[mode] = dict(x=x, xn=xn, stats=stats, qkv=qkv, o=o)
            x = x_new
        g, b_, w1, b1, w2, b2 = next(it), next(it), next(it), next(it), next(it), next(it)
        if last and prune_last:
            # feed-forward block on the cls rows only (x is [B, D] here)
            xn_c, h_c, stats_c = _new(dev, B, D), _new(dev, B, 4 * D), (_new(dev, B, 2) if save else None)
            u_c = _new(dev, B, 8 * D) if save else None
            L.mt.layernorm_fwd(x, g, b_, xn_c, stats_c, B, D, eps, None)
            L.gemm(L.OP_NT, xn_c, w1, h_c, B, 8 * D, D, D, D, 4 * D, epilogue=L.EPI_GEGLU, bias=b1, C2=u_c, ldc2=8 * D, n_half=4 * D)
            x_out = _new(dev, B, 1, D)
            L.gemm(L.OP_NT, h_c, w2, x_out, B, D, 4 * D, 4 * D, 4 * D, D, epilogue=L.EPI_BIAS_RES, bias=b2, R=x, ldr=D)
            if save:
                rec[2] = dict(x=x, xn=xn_c, stats=stats_c, u=u_c, h=h_c)
                saved["layers"].append(rec)
                saved["pruned_last"] = True
            x = x_out
            continue
        if save:
            xn, hbuf, stats = _new(dev, M, D), _new(dev, M, 4 * D), _new(dev, M, 2)
            u = _new(dev, M, 8 * D)
        else:
            stats, u = None, None
        L.mt.layernorm_fwd(x, g, b_, xn, stats, M, D, eps, None)
        L.gemm(L.OP_NT, xn, w1, hbuf, M, 8 * D, D, D, D, 4 * D, epilogue=L.EPI_GEGLU, bias=b1, C2=u, ldc2=8 * D, n_half=4 * D)
        x_new = _new(dev, B, N, D) if save else x
        L.gemm(L.OP_NT, hbuf, w2, x_new, M, D, 4 * D, 4 * D, 4 * D, D, epilogue=L.EPI_BIAS_RES, bias=b2, R=x, ldr=D)
        if save:
            rec[2] = dict(x=x, xn=xn, stats=stats, u=u, h=hbuf)
            saved["layers"].append(rec)
        x = x_new
    g, b_, w_h, b_h = next(it), next(it), next(it), next(it)
    logits = _new(dev, B, model.num_classes)
    L.mt.head_fwd(x, g, b_, w_h, b_h, logits, B, x.shape[1], D, model.num_classes, eps)    # x: [B, N, D], or [B, 1, D] after pruning
    if save:
        saved["x_final"] = x
    return logits, s_att, t_att, saved


_AUX = ("mask", "ident", "sizes", "positions")       # the per-clip side inputs a recorded forward reads from static buffers


class _TSFFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, aux, dims, feat, *params):
        B, F, n, grad_on = dims
        dims = (B, F, n)
        # needs_input_grad mirrors requires_grad even under torch.no_grad(), and grad mode is always off inside forward():
        # the caller's grad mode comes in through `dims`.  Without it an eval forward would keep every activation.
        save = grad_on and any(ctx.needs_input_grad)
        ctx.model, ctx.dims, ctx.params = model, dims, params
        planes = tsf_planes.eligible(model, B * (1 + F * n), save)
        stream = key = None
        if planes and save and not tsf_planes.dropout_active(model):
            stream = torch.cuda.current_stream(feat.device).cuda_stream
            key = ("tsf", B, F, n, feat.dtype, model.training, model.require_attention, L.deterministic(),
                   tuple(ctx.needs_input_grad[3:]), stream, os.environ.get("MT_PLANES_STREAMK", "0"),
                   tuple(getattr(aux, nm) is None for nm in _AUX), tsf_planes.prune_last(model, B))

        def body(ins, plan):
            a = aux if plan is None else types.SimpleNamespace(err=aux.err, **{nm: ins["aux_" + nm] for nm in _AUX})
            if planes:
                logits, s_att, t_att, saved = tsf_planes.tsf_forward_planes(model, ins["feat"], a, params, B, F, n, save)
            elif tsf_planes.dropout_active(model):
                raise NotImplementedError("attn-dropout / ff-dropout > 0 in train mode runs on the plane path only (MT_TSF_PLANES=1, "
                                          "MT_GEMM_SPLIT=1, not under stream capture)")
            else:
                logits, s_att, t_att, saved = tsf_forward(model, ins["feat"], a, params, B, F, n, save)
            if saved is not None:
                saved.update(feat=ins["feat"], aux=a)        # what the backward reads besides its activations
            return (logits, s_att, t_att), saved
        inputs = {"feat": feat, **{"aux_" + nm: getattr(aux, nm) for nm in _AUX}}
        # a plan's user-facing outputs are small ([B, classes], two [(B H), 1, N] maps): handed out as copies, so that a caller who keeps
        # predictions on the device across steps does not see the next replay write over them (the eager path returns fresh tensors)
        logits, s_att, t_att = plans.forward(ctx, model, key, stream, params, inputs, body, clone_outputs=True,
                                             after_run=lambda np_: _publish_index_flag(aux.err))
        if model.require_attention:
            ctx.mark_non_differentiable(s_att, t_att)
            return logits, s_att, t_att
        return (logits,)

    @staticmethod
    def backward(ctx, dlogits, *unused):
        s = ctx.saved
        need_df, need_dp = ctx.needs_input_grad[3], ctx.needs_input_grad[4:]

        def body(g, keep_saved, plan):
            if s.get("planes"):
                dfeat, dparams = tsf_planes.tsf_backward_planes(ctx.model, s["feat"], s["aux"], ctx.params, ctx.dims, s, g, need_df,
                                                                need_dp, keep_saved=keep_saved, plan=plan)
            else:
                dfeat, dparams = tsf_backward(ctx.model, s["feat"], s["aux"], ctx.params, ctx.dims, s, g, need_df, need_dp)
            return (dfeat,), dparams
        return (None, None, None) + plans.backward(ctx, "SizeInvariantTimeSformer", dlogits.contiguous(), body)


def tsf_apply(model, x, mask, identities_mask, size_embedding, positions):
    if not x.is_cuda:
        raise L.MintimeHipError("SizeInvariantTimeSformer (MI355X build) needs device tensors; there is no CPU path")
    b, f, c, h, w = x.shape
    if c != model.channels:
        raise ValueError(f"expected {model.channels} feature channels, got {c}")
    if f != model.num_frames:
        raise ValueError(f"expected num-frames={model.num_frames} face slots per clip, got {f}")
    if h * w != model.num_patches:
        raise ValueError(f"expected {model.num_patches} patches per slot, got {h * w}")
    grad_on = torch.is_grad_enabled()
    aux = _Aux(model, x, mask, identities_mask, size_embedding, positions)
    outs = _TSFFunction.apply(model, aux, (b, f, h * w, grad_on), _as_tokens(x.float()), *model._param_list())
    if model.require_attention:
        return outs[0], [outs[1], outs[2]]       # order [space, time] (reference :271)
    return outs[0]
