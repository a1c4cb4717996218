"""Launch sequences (forward and backward) of Xception on libmintime_hip (reference models/xception.py:161-217).

Same rules as the EfficientNet engine: NHWC rows, raw conv outputs in HBM with BatchNorm(+ReLU) applied by the consumer on
load, BatchNorm statistics accumulated by the producer, BatchNorm backward folded into GEMM operand loads.
A `_Src` describes how a consumer obtains a tensor's value: stored data + pending per-channel affine + pending activation.
"""
import torch

from . import arch
from . import lib as L
from . import plans
from .effnet_engine import SLOTS, _StatsPool, _BNCtx, _finalize, _bump_tracked
from .lib import _new

RELU, NONE = 2, 0


# pointwise convolutions with at least this many input channels run on plane operands (MT_GEMM_SPLIT=0: none does, all take mt_gemm)
PLANES_MIN_C = 256   # (128: +0.4 ms in config 5 once the 4 GB operand limit is respected, lib.planes_fit)
DW_PLANES = __import__("os").environ.get("MT_XC_DW_PLANES", "1") != "0"   # 0: depthwise output as fp32 + mt_split_planes_blk (round 4)
# share (of the images) of conv2's weight gradient on the side stream (round 5: 1.0: 203.0 ms, 0.7: 201.7 on one box; round 6 with the
# one-tile weight gradient: 0.5 / 0.7 / 1.0 within 0.6 ms)
CONV2_WGRAD_SIDE = 0.7
SKIP_HALF = __import__("os").environ.get("MT_XC_SKIP_HALF", "1") != "0"    # 0: the skip path's data gradient scattered into a zeroed full-size tensor
POOL_ARG = __import__("os").environ.get("MT_XC_POOL_ARG", "1") != "0"      # 0: the adjoint of the max-pool as an arg-max scatter (round 4)


class _Src:
    def __init__(self, t, C, H, scale=None, shift=None, act=NONE, bn=None):
        self.t, self.C, self.H, self.scale, self.shift, self.act, self.bn = t, C, H, scale, shift, act, bn


class _Consts:
    """ones / zeros vectors for tensors that carry no pending affine (the depthwise kernels always take scale/shift)."""

    def __init__(self, dev):
        self.dev, self.cache = dev, {}

    def ident(self, C):
        if C not in self.cache:
            self.cache[C] = (torch.ones(C, device=self.dev), torch.zeros(C, device=self.dev))
        return self.cache[C]

    def kabc_ident(self, C):
        key = ("k", C)
        if key not in self.cache:
            k = torch.zeros(3, C, device=self.dev)
            k[0] = 1.0
            self.cache[key] = k
        return self.cache[key]


def param_list(model):
    ps = [model.conv1.weight, model.bn1.weight, model.bn1.bias, model.conv2.weight, model.bn2.weight, model.bn2.bias]
    for blk in model.blocks():
        if blk.skip is not None:
            ps += [blk.skip.weight, blk.skipbn.weight, blk.skipbn.bias]
        for (i_sep, i_bn, ci, co) in blk.unit_index:
            sep, bn = getattr(blk.rep, str(i_sep)), getattr(blk.rep, str(i_bn))
            ps += [sep.conv1.weight, sep.pointwise.weight, bn.weight, bn.bias]
    for sep, bn in ((model.conv3, model.bn3), (model.conv4, model.bn4)):
        ps += [sep.conv1.weight, sep.pointwise.weight, bn.weight, bn.bias]
    return ps


def _total_channels(model):
    c = 32 + 64 + 1536 + 2048
    for blk in model.blocks():
        if blk.skip is not None:
            c += blk.cfg[2]
        c += sum(co for (_, _, _, co) in blk.unit_index)
    return c


class _WeightPlanes:
    """Plane tensors of the pointwise-conv weights that run on plane operands.  The first forward splits them one by one and registers
    them; every later forward re-splits all of them with ONE mt_split_planes_blk_multi launch (33 launches per step before)."""

    def __init__(self):
        self.items = {}          # weight data_ptr -> (weight, planes, co, ci)
        self.table = None
        self.fresh = False
        self.serial = plans.PlaneSerial("the pointwise weights")

    def begin(self, lib):
        self.fresh = False
        if self.table is None:
            return
        if any(w.data_ptr() != k for k, (w, _, _, _) in self.items.items()):       # a weight moved: start over
            self.items, self.table = {}, None
            return
        L.mt.split_planes_blk_multi(self.table, len(self.items), self.blocks)
        self.fresh = True

    def get(self, w_pw, co, ci):
        ent = self.items.get(w_pw.data_ptr())
        if ent is not None and self.fresh and ent[0] is w_pw:
            return ent[1]
        planes = L.split_planes_blk(w_pw.view(co, ci), co, ci)
        self.items[w_pw.data_ptr()] = (w_pw, planes, co, ci)
        self.table = None
        return planes

    def end(self, dev):
        if self.table is not None or not self.items:
            return
        rows, first = [], 0
        for k, (w, pl, co, ci) in self.items.items():
            rows.append((k, pl.data_ptr(), co, ci, first))
            first += pl.shape[1] * pl.shape[2]
        self.host = torch.tensor(rows, dtype=torch.int64).pin_memory()
        self.table = self.host.to(dev, non_blocking=True)
        self.blocks = first


def xception_forward(model, x, params, training, save, plan=None):
    """plan: the plans.NetPlan being recorded (it keeps the tracked counters for its replays)."""
    lib = L.get()
    dev = x.device
    N, H, W, _ = x.shape
    det = training and L.deterministic()
    pool = _StatsPool(dev, _total_channels(model), det) if training else None
    consts = _Consts(dev)
    slots = -SLOTS if det else SLOTS          # deterministic mode: BatchNorm sums as integer limbs -- order-independent, no second pass
    epi = L.EPI_STATS if training else L.EPI_STORE
    planes_on = L.gemm_split_enabled()
    wplanes = model.__dict__.setdefault("_xc_wplanes", _WeightPlanes())
    if planes_on:
        wplanes.begin(lib)
    it = iter(params)
    saved = {"x": x, "blocks": [], "consts": consts} if save else None

    def pack(w, Co, Ci, k, ld, transpose=0):
        out = _new(dev, Ci if transpose else Co, ld)
        L.mt.conv_weight_pack(w, out, Co, Ci, k, ld, transpose)
        return out

    def conv_im2col(src, wp, Cout, K, geom, bn_mod, gamma, beta, u8=False):
        """z = im2col(act(affine(src))) . wp^T  (+ BatchNorm statistics)."""
        Hh, Ww, Cc, Ho, Wo, k, s_, p_ = geom
        M = N * Ho * Wo
        ctx = _BNCtx(dev, Cout, training, pool)
        z = _new(dev, M, Cout)
        L.gemm(L.OP_NT, src.t, wp, z, M, Cout, K, K, K, Cout, prologue=L.PRO_IM2COL, epilogue=epi, scale=src.scale, shift=src.shift,
               stats=ctx.stats, stats_slots=slots, conv=(Hh, Ww, Cc, Ho, Wo, k, s_, p_, src.act, 1 if u8 else 0))
        _finalize(bn_mod, ctx, M, training, gamma, beta, slots)
        return z, ctx

    def sep_unit(src, act, w_dw, w_pw, co, bn_mod, gamma, beta):
        """[act] -> depthwise 3x3 pad 1 -> pointwise 1x1 -> BatchNorm (xception.py:17-27, 44-58)."""
        Hh, ci = src.H, src.C
        M = N * Hh * Hh
        sc, sh = (src.scale, src.shift) if src.scale is not None else consts.ident(ci)
        eff = RELU if (act == RELU or src.act == RELU) else NONE
        ctx = _BNCtx(dev, co, training, pool)
        z = _new(dev, M, co)
        d = d_p = w_p = None
        if planes_on and ci >= PLANES_MIN_C and M >= 512 and L.planes_fit(M, max(ci, co)):
            # wide pointwise convolutions on plane operands (csrc/gemm_planes.hpp): forward, data gradient and weight gradient read
            # the same plane tensors by LDS-DMA (728 -> 728 over 100 352 rows: 0.81 -> 0.58 ms).  The weight is split once per
            # forward; the depthwise kernel writes its output as planes and nowhere else (DW_PLANES; round 4: fp32 + a split pass)
            d_p = L.planes_empty(M, ci, dev)
            if DW_PLANES:
                L.mt.dwconv_fwd_planes(src.t, sc, sh, w_dw, d_p, N, Hh, Hh, ci, 3, 1, eff)
            else:
                d = _new(dev, M, ci)
                L.mt.dwconv_fwd(src.t, sc, sh, w_dw, d, None, SLOTS, N, Hh, Hh, ci, 3, 1, eff)
                L.split_planes_blk(d, M, ci, out=d_p)
                d = None                                   # backward reads d through its planes only
            w_p = wplanes.get(w_pw, co, ci)
            L.gemm_planes(L.OP_NT, d_p, w_p, M, co, ci, Cout=z, ldc=co, epilogue=epi, stats=ctx.stats, stats_slots=slots)
        else:
            d = _new(dev, M, ci)
            L.mt.dwconv_fwd(src.t, sc, sh, w_dw, d, None, SLOTS, N, Hh, Hh, ci, 3, 1, eff)
            L.gemm(L.OP_NT, d, w_pw, z, M, co, ci, ci, ci, co, epilogue=epi, stats=ctx.stats, stats_slots=slots)
        _finalize(bn_mod, ctx, M, training, gamma, beta, slots)
        rec = dict(src=src, eff=eff, sc=sc, sh=sh, d=d, d_p=d_p, w_p=w_p, z=z, bn=ctx, ci=ci, co=co, H=Hh) if save else None
        return _Src(z, co, Hh, ctx.scale, ctx.shift, NONE, ctx), rec

    # ---- conv1 (3x3 s2 p0, 3 -> 32) and conv2 (3x3 s1 p0, 32 -> 64) as im2col GEMMs
    w1, g1, b1, w2, g2, b2 = next(it), next(it), next(it), next(it), next(it), next(it)
    H1 = (H - 3) // 2 + 1
    if W <= 512:
        # conv1 = the EfficientNet stem's streaming MFMA kernel without padding (K = 27 is far too short for the im2col GEMM: 4.3 ms
        # against 0.5 at 512 crops); reads uint8 crops as well
        bn1 = _BNCtx(dev, 32, training, pool)
        z1 = _new(dev, N * H1 * H1, 32)
        L.mt.stem_conv_fwd_valid(x, 1 if x.dtype == torch.uint8 else 0, w1, z1, bn1.stats if training else None, slots, N, H, W)
        _finalize(model.bn1, bn1, N * H1 * H1, training, g1, b1, slots)
    else:
        wp1 = pack(w1, 32, 3, 3, 28)
        z1, bn1 = conv_im2col(_Src(x, 3, H), wp1, 32, 28, (H, W, 3, H1, H1, 3, 2, 0), model.bn1, g1, b1, u8=x.dtype == torch.uint8)
    s1 = _Src(z1, 32, H1, bn1.scale, bn1.shift, RELU, bn1)
    H2 = H1 - 2
    wp2 = pack(w2, 64, 32, 3, 288)
    z2, bn2 = conv_im2col(s1, wp2, 64, 288, (H1, H1, 32, H2, H2, 3, 1, 0), model.bn2, g2, b2)
    cur = _Src(z2, 64, H2, bn2.scale, bn2.shift, RELU, bn2)
    if save:
        saved.update(z1=z1, bn1=bn1, s1=s1, z2=z2, bn2=bn2, H1=H1, H2=H2)

    # ---- blocks
    for blk in model.blocks():
        name, cin, cout, reps, stride, srelu, grow = blk.cfg
        inp = cur
        brec = {"inp": inp, "units": [], "stride": stride}
        if blk.skip is not None:
            w_s, g_s, b_s = next(it), next(it), next(it)
        src = cur
        for u, (i_sep, i_bn, ci, co) in enumerate(blk.unit_index):
            w_dw, w_pw, g, b = next(it), next(it), next(it), next(it)
            act = RELU if (u > 0 or srelu) else NONE
            src, rec = sep_unit(src, act, w_dw, w_pw, co, getattr(blk.rep, str(i_bn)), g, b)
            brec["units"].append(rec)
        Hin = inp.H
        if stride != 1:
            Ho = (Hin - 1) // 2 + 1
            z_s, bn_s = conv_im2col(inp, w_s.view(cout, cin), cout, cin, (Hin, Hin, cin, Ho, Ho, 1, 2, 0), blk.skipbn, g_s, b_s)
            y = _new(dev, N * Ho * Ho, cout)
            if save and POOL_ARG:
                # the adjoint's routing is recorded here (1 byte + the raw arg-max value per pooled element): backward never builds the
                # full-resolution routed gradient by atomics, and takes the pooled unit's BatchNorm sums from the pooled tensors
                arg = torch.empty(N * Ho * Ho, cout, dtype=torch.uint8, device=dev)
                zmax = _new(dev, N * Ho * Ho, cout)
                L.mt.maxpool_add_fwd_arg(src.t, src.scale, src.shift, z_s, bn_s.scale, bn_s.shift, y, arg, zmax, N, Hin, Hin, cout)
                brec.update(arg=arg, zmax=zmax)
            else:
                L.mt.maxpool_add_fwd(src.t, src.scale, src.shift, z_s, bn_s.scale, bn_s.shift, y, N, Hin, Hin, cout)
            brec.update(z_s=z_s, bn_s=bn_s, Ho=Ho)
            cur = _Src(y, cout, Ho)
        else:
            y = _new(dev, N * Hin * Hin, cout)
            L.mt.bn_act_fwd(src.t, src.scale, src.shift, inp.t, y, N * Hin * Hin, cout, 0, None, 1)
            cur = _Src(y, cout, Hin)
        if save:
            saved["blocks"].append(brec)

    # ---- conv3 / conv4 tail
    tail = []
    for k_, (sep_mod, bn_mod, co, act) in enumerate(((model.conv3, model.bn3, 1536, NONE), (model.conv4, model.bn4, 2048, RELU))):
        w_dw, w_pw, g, b = next(it), next(it), next(it), next(it)
        cur, rec = sep_unit(cur, act, w_dw, w_pw, co, bn_mod, g, b)
        tail.append(rec)
    M = N * cur.H * cur.H
    feat = _new(dev, M, 2048)
    L.mt.bn_act_fwd(cur.t, cur.scale, cur.shift, None, feat, M, 2048, 0, None, 1)
    if save:
        saved["tail"] = tail
    if planes_on:
        wplanes.end(dev)
        w_serial = wplanes.serial.touch([w for w, _, _, _ in wplanes.items.values()])
        if save:
            saved["w_serial"] = w_serial
    _bump_tracked(plan)
    return feat, saved, cur.H


def xception_backward(model, params, saved, shape, training, dfeat, need_dparams, keep_saved=False, plan=None, need_dx=False):
    """Returns (gradient w.r.t. the crops [N,H,W,3] or None, parameter gradients).  keep_saved: the activation records belong to a
    launch plan (plans.py) and stay for its next replay; plan: the NetPlan whose backward phase is being recorded (it keeps the flat
    gradient buffer); need_dx: the crops require grad (the walk ends with mt_stem_conv_dgrad_valid)."""
    lib = L.get()
    dev = dfeat.device
    N, H, W = shape
    P = list(params)
    grads, flat_grads = L.zero_grads(P, with_flat=True)
    consts = saved["consts"]
    det = L.deterministic()
    slots = -SLOTS if det else SLOTS          # (see xception_forward)
    pool = _StatsPool(dev, 2 * _total_channels(model) + 4096, det)
    tr = 1 if training else 0
    side = L.SideStream(dev, hold=True)
    # parameter index map
    pos = 6
    bmap = []
    for blk in model.blocks():
        d = {}
        if blk.skip is not None:
            d["skip"] = pos
            pos += 3
        d["units"] = []
        for _ in blk.unit_index:
            d["units"].append(pos)
            pos += 4
        bmap.append(d)
    tail_idx = [pos, pos + 4]

    def bn_sums(g, z, ctx, rows, act=0, dout=None):
        sums = pool.take(ctx.C)
        L.mt.bn_act_bwd(g, z, ctx.scale, ctx.shift, ctx.mean_invstd, None, None, None, dout, sums, slots, rows, ctx.C, 1, act)
        return sums

    def bn_kabc(ctx, sums, gi, d, z, rows):
        """(d, z, rows): the gradient w.r.t. the BatchNorm's output and its input tensor (round 4's deterministic mode retook the sums
        from them; they are integer limbs now)."""
        kabc = _new(dev, 3, ctx.C)
        L.mt.bn_bwd_finalize(sums, slots, ctx.count, P[gi], ctx.mean_invstd, kabc, grads[gi], grads[gi + 1], ctx.C, tr)
        return kabc

    def unit_backward(rec, pi, g, sums, res_pre=None, res_post=None, pooled=None, res_half=False):
        """g = gradient w.r.t. this unit's BatchNorm output (sums already accumulated when `sums` is given).
        pooled = (dy, arg, zmax, Ho) instead of g: the unit feeds the block's max-pool and the gradient is dy routed by `arg`.
        res_half: res_pre / res_post are at half resolution (the stride-2 skip convolution's data gradient, even positions only).
        Returns (gradient w.r.t. the source's affine output [activation derivative applied], its BN sums or None)."""
        ci, co, Hh = rec["ci"], rec["co"], rec["H"]
        M = N * Hh * Hh
        if pooled is not None:
            p_dy, p_arg, p_zmax, p_Ho = pooled
            sums = bn_sums(p_dy, p_zmax, rec["bn"], N * p_Ho * p_Ho)      # sum du = sum dy, sum du xhat = sum dy xhat(arg-max)
            if rec["d_p"] is None:
                g = _new(dev, M, co)
                L.mt.maxpool_bwd_arg(p_dy, p_arg, g, N, Hh, Hh, co)
        elif sums is None:
            sums = bn_sums(g, rec["z"], rec["bn"], M)
        kabc = bn_kabc(rec["bn"], sums, pi + 2, g, rec["z"], M)
        w_dw, w_pw = P[pi], P[pi + 1]
        # pointwise: z = d . Wpw^T
        dd = _new(dev, M, ci)
        if rec["d_p"] is not None:
            # plane operands: dz = ka g + kb z + kc is evaluated ONCE, as planes, and feeds both gradient GEMMs
            dz_p = L.planes_empty(M, co, dev)
            if pooled is not None:
                L.mt.maxpool_bn_bwd_apply_planes(p_dy, p_arg, rec["z"], kabc, dz_p, N, Hh, Hh, co)
            else:
                L.mt.bn_bwd_apply_planes(g, rec["z"], kabc, dz_p, M, co)
            side.launch(lambda: L.gemm_planes(L.OP_TN, dz_p, rec["d_p"], co, ci, M, Cout=grads[pi + 1].view(co, ci), ldc=ci,
                                              epilogue=L.EPI_ATOMIC), reads=(dz_p, rec["d_p"]))
            L.gemm_planes(L.OP_NN, dz_p, rec["w_p"], M, ci, co, Cout=dd, ldc=ci)
        else:
            side.launch(lambda: L.gemm(L.OP_TN, g, rec["d"], grads[pi + 1], co, ci, M, co, ci, ci, prologue=L.PRO_BN_BWD,
                                       epilogue=L.EPI_ATOMIC, split_k=0, A2=rec["z"], scale=kabc[0], shift=kabc[1], gate=kabc[2]),
                        reads=(g, rec["d"], rec["z"], kabc))
            L.gemm(L.OP_NN, g, w_pw, dd, M, ci, co, co, ci, ci, prologue=L.PRO_BN_BWD, A2=rec["z"], scale=kabc[0], shift=kabc[1],
                   gate=kabc[2])
        # depthwise: d = dw(act(affine(src)))
        src = rec["src"]
        kid = consts.kabc_ident(ci)
        has_bn = src.bn is not None
        sums_in = pool.take(ci) if has_bn else None
        du_in = _new(dev, M, ci)

        def dw_part(parts):
            fn = L.mt.dwconv_bwd_res2 if res_half else L.mt.dwconv_bwd
            fn(dd, dd, kid, w_dw, src.t, rec["sc"], rec["sh"], src.bn.mean_invstd if has_bn else None, du_in, sums_in, slots, grads[pi],
               N, Hh, Hh, ci, 3, 1, parts, rec["eff"], res_pre, res_post)
        if not det:
            # data + weight gradient from one pass (effnet_backward.FUSED_DW; all of Xception's depthwise layers are 3x3 stride 1):
            # config 5 200.0 -> 193.5 ms.  Deterministic mode keeps the two kernels on two streams (the logged weight-gradient kernel)
            dw_part(3)
        else:
            side.launch(lambda: dw_part(1), reads=(dd, kid, src.t, rec["sc"], rec["sh"]))
            dw_part(2)
        return du_in, sums_in

    # ---- tail: feat = bn4(z4); conv4 consumes relu(bn3(z3)); conv3 consumes y12 (no relu)
    t3, t4 = saved["tail"]
    g, sums = unit_backward(t4, tail_idx[1], dfeat, None)            # -> grad wrt bn3 output (+ bn3 sums)
    dy, _ = unit_backward(t3, tail_idx[0], g, sums)                  # -> grad wrt y12

    # ---- blocks, last to first
    blocks = model.blocks()
    for bi in reversed(range(len(blocks))):
        blk, brec, bm = blocks[bi], saved["blocks"][bi], bmap[bi]
        name, cin, cout, reps, stride, srelu, grow = blk.cfg
        inp = brec["inp"]
        units = brec["units"]
        last = units[-1]
        Hin = inp.H
        res_pre = res_post = None
        if stride != 1:
            Ho = brec["Ho"]
            Mo = N * Ho * Ho
            # skip path: y += skipbn(z_s), z_s = conv1x1_s2(value of inp)
            ks = bn_kabc(brec["bn_s"], bn_sums(dy, brec["z_s"], brec["bn_s"], Mo), bm["skip"] + 1, dy, brec["z_s"], Mo)
            geom = (Hin, Hin, cin, Ho, Ho, 1, 2, 0, inp.act)
            side.launch(lambda dy=dy, ks=ks, brec=brec, geom=geom, inp=inp, gi=bm["skip"]:
                        L.gemm(L.OP_TN, dy, inp.t, grads[gi].view(cout, cin), cout, cin, Mo, cout, cin, cin, prologue=L.PRO_BN_BWD,
                               epilogue=L.EPI_ATOMIC, split_k=0, A2=brec["z_s"], scale=ks[0], shift=ks[1], gate=ks[2],
                               b_prologue=L.BPRO_IM2COL, b_scale=inp.scale, b_shift=inp.shift, conv=geom),
                        reads=(dy, inp.t, brec["z_s"], ks))
            d_small = _new(dev, Mo, cin)
            L.gemm(L.OP_NN, dy, P[bm["skip"]].view(cout, cin), d_small, Mo, cin, cout, cout, cin, cin, prologue=L.PRO_BN_BWD,
                   A2=brec["z_s"], scale=ks[0], shift=ks[1], gate=ks[2])
            # it lands on the even positions (2oh, 2ow) of the block input: the first unit's depthwise adjoint adds it from the
            # half-resolution tensor (SKIP_HALF; round 4 scattered it into an input-sized zero tensor first)
            if SKIP_HALF:
                d_skip = d_small
            else:
                d_skip = torch.zeros(N, Hin, Hin, cin, dtype=torch.float32, device=dev)
                d_skip[:, ::2, ::2, :] = d_small.view(N, Ho, Ho, cin)
                d_skip = d_skip.view(N * Hin * Hin, cin)
            if inp.bn is not None or inp.act == RELU:
                res_pre = d_skip          # the skip conv consumed the same activated tensor as the first unit
            else:
                res_post = d_skip         # the skip conv consumed the raw block input, the first unit relu(input)
            # main path: y += maxpool(bn(z_last))
            pooled = None
            if "arg" in brec:
                g, sums, pooled = None, None, (dy, brec["arg"], brec["zmax"], Ho)
            else:
                du_last = torch.zeros(N * Hin * Hin, cout, dtype=torch.float32, device=dev)
                L.mt.maxpool_bwd(dy, last["z"], last["bn"].scale, last["bn"].shift, du_last, N, Hin, Hin, cout)
                g, sums = du_last, None
        else:
            g, sums, pooled = dy, None, None
            res_post = dy                 # identity skip: y = bn(z_last) + inp
        for u in reversed(range(len(units))):
            first = u == 0
            g, sums = unit_backward(units[u], bm["units"][u], g, sums, res_pre if first else None, res_post if first else None,
                                    pooled if u == len(units) - 1 else None, res_half=first and stride != 1 and SKIP_HALF)
        # for block1 the result is the gradient w.r.t. bn2's output (sums accumulated); otherwise w.r.t. the previous block's y
        dy = g
        bn2_sums = sums
        if not keep_saved:
            brec.clear()
        side.release_point()

    # ---- conv2 / conv1
    z1, z2, bn1, bn2, s1 = saved["z1"], saved["z2"], saved["bn1"], saved["bn2"], saved["s1"]
    H1, H2 = saved["H1"], saved["H2"]
    M1, M2 = N * H1 * H1, N * H2 * H2
    k2 = bn_kabc(bn2, bn2_sums, 4, dy, z2, M2)
    dwp2 = L.zeros((64, 288), torch.float32, dev)          # (a fill of the library: a recorded phase re-issues it)
    geom2 = (H1, H1, 32, H2, H2, 3, 1, 0, RELU)

    def conv2_wgrad(n0, n1):      # images [n0, n1): 6 M rows x (64 x 288) in all, 9 ms
        r0, r1 = n0 * H2 * H2, n1 * H2 * H2
        L.gemm(L.OP_TN, dy[r0:r1], z1[n0 * H1 * H1:n1 * H1 * H1], dwp2, 64, 288, r1 - r0, 64, 288, 288, prologue=L.PRO_BN_BWD,
               epilogue=L.EPI_ATOMIC, split_k=0, A2=z2[r0:r1], scale=k2[0], shift=k2[1], gate=k2[2], b_prologue=L.BPRO_IM2COL,
               b_scale=bn1.scale, b_shift=bn1.shift, conv=geom2)
    # most of it on the side stream, beside conv2's data gradient and conv1's weight gradient; the rest after those on the main stream,
    # so that both queues end together (the whole of it on either queue leaves the other idle for 3-9 ms at the end of the step)
    # (deterministic mode: every split-K GEMM of this backward stays on the side stream -- they share the slab arena in stream order)
    n_side = N if (not side.enabled or det) else max(1, min(N, int(round(N * CONV2_WGRAD_SIDE))))
    side.launch(lambda: conv2_wgrad(0, n_side), reads=(dy, z1, z2, k2, dwp2, bn1.scale, bn1.shift))
    dz2 = _new(dev, M2, 64)
    L.mt.bn_bwd_apply(dy, z2, k2, dz2, M2, 64)
    # data gradient of conv2 = "full" correlation of dz2 with the flipped kernel: im2col(dz2, pad 2) . W2flip^T
    wp2t = _new(dev, 32, 576)
    L.mt.conv_weight_pack(P[3], wp2t, 64, 32, 3, 576, 1)
    da1 = _new(dev, M1, 32)
    L.gemm(L.OP_NT, dz2, wp2t, da1, M1, 32, 576, 576, 576, 32, prologue=L.PRO_IM2COL, conv=(H2, H2, 64, H1, H1, 3, 1, 2, NONE))
    du1 = _new(dev, M1, 32)
    k1 = bn_kabc(bn1, bn_sums(da1, z1, bn1, M1, act=RELU, dout=du1), 1, du1, z1, M1)
    dx = None
    if need_dx:
        if W > 512:
            raise NotImplementedError("gradient w.r.t. the input crops: mt_stem_conv_dgrad_valid takes crops of at most 512 columns")
        # the last operator of the walk: the transposed conv1, 32 -> 3 channels (csrc/stem_dgrad.hip)
        dx = _new(dev, N, H, W, 3)
        L.mt.stem_conv_dgrad_valid(du1, z1, k1, P[0], dx, N, H, W)
    if W <= 512:
        L.mt.stem_conv_wgrad_valid(du1, z1, k1, saved["x"], 1 if saved["x"].dtype == torch.uint8 else 0, grads[0], N, H, W)
    else:
        dwp1 = torch.zeros(32, 28, dtype=torch.float32, device=dev)
        L.gemm(L.OP_TN, du1, saved["x"], dwp1, 32, 28, M1, 32, 28, 28, prologue=L.PRO_BN_BWD, epilogue=L.EPI_ATOMIC, split_k=0, A2=z1,
               scale=k1[0], shift=k1[1], gate=k1[2], b_prologue=L.BPRO_IM2COL,
               conv=(H, W, 3, H1, H1, 3, 2, 0, NONE, 1 if saved["x"].dtype == torch.uint8 else 0))
        L.mt.conv_weight_unpack_grad(dwp1, grads[0], 32, 3, 3, 28)
    if n_side < N:
        conv2_wgrad(n_side, N)
    side.wait()
    L.mt.conv_weight_unpack_grad(dwp2, grads[3], 64, 32, 3, 288)
    if plan is not None:
        plan.extra["flat_grads"] = flat_grads
    L.grads_ready(model, P, flat_grads)
    return dx, [g_ if need else None for need, g_ in zip(need_dparams, grads)]


def _plannable():
    """The recorded form covers the default kernels only: the lab alternatives issue torch fills / scatters a recording cannot see."""
    return SKIP_HALF and POOL_ARG and DW_PLANES


class _XceptionFunction(torch.autograd.Function):
    """Forward / backward of the extractor; like effnet_engine._EffNetFunction the two launch sequences are recorded into the library
    the second time a (shape, mode) key is seen and re-issued from C afterwards (plans.py): ~750 ctypes launches per step become 2."""

    @staticmethod
    def forward(ctx, model, x_nhwc, *params):
        model, grad_on = model
        save = grad_on and any(ctx.needs_input_grad)      # see tsf_engine._TSFFunction.forward
        N, H, W, _ = x_nhwc.shape
        ctx.shape = (N, H, W)
        ctx.model, ctx.params, ctx.training = model, params, model.training
        stream = key = state = None
        # (crops that require grad run the eager launch sequence: plan keys do not carry them)
        if save and _plannable() and W <= 512 and L.gemm_split_enabled() and not ctx.needs_input_grad[1]:
            stream = torch.cuda.current_stream(x_nhwc.device).cuda_stream
            state = list(params) + list(model.buffers())       # (what a recording holds the addresses of)
            key = ("xc", tuple(x_nhwc.shape), x_nhwc.dtype, model.training, L.deterministic(), tuple(ctx.needs_input_grad[2:]), stream,
                   float(model.bn1.momentum), float(model.bn1.eps))

        def body(ins, plan):
            feat, saved, _ = xception_forward(model, ins["x"], params, model.training, save, plan=plan)
            return (feat,), saved
        feat, = plans.forward(ctx, model, key, stream, state, {"x": x_nhwc}, body)
        return feat

    @staticmethod
    def backward(ctx, dfeat):
        def body(g, keep_saved, plan):
            dx, dparams = xception_backward(ctx.model, ctx.params, ctx.saved, ctx.shape, ctx.training, g, ctx.needs_input_grad[2:],
                                            keep_saved=keep_saved, plan=plan, need_dx=ctx.needs_input_grad[1])
            return (dx,), dparams
        return (None,) + plans.backward(ctx, "Xception", dfeat.contiguous(), body)


def xception_apply(model, inputs):
    if not inputs.is_cuda:
        raise L.MintimeHipError("Xception (MI355X build) needs device tensors; there is no CPU path")
    if inputs.dim() != 4 or inputs.shape[1] != 3:
        raise ValueError(f"expected [N,3,H,W] input, got {tuple(inputs.shape)}")
    x = (inputs if inputs.dtype == torch.uint8 else inputs.float()).permute(0, 2, 3, 1)      # uint8 crops are ingested as they are
    if not x.is_contiguous():
        x = x.contiguous()
    feat = _XceptionFunction.apply((model, torch.is_grad_enabled()), x, *param_list(model))
    n = inputs.shape[0]
    ho = feat.shape[0] // n
    side = int(round(ho ** 0.5))
    return feat.view(n, side, side, 2048).permute(0, 3, 1, 2)
