"""SlowFast R50 layer walk on libmintime_hip: one torch.autograd.Function over the whole network (slowfast.py).

Activations are channels-last rows ([N*T*H*W, C] tensors, possibly a column slice of a wider one).  The forward keeps the raw
convolution outputs (pre-BatchNorm z) and every block output; BatchNorm + ReLU of a convolution's producer is applied on the
consumer's loads (mt_conv3d_* prologue), so relu(bn(z)) is only materialised at block outputs and stem pools.  Each fusion
convolution writes its raw output straight into the channel tail of the slow pathway's concatenated tensor; the consumers of that
tensor apply (scale, shift) = (1, 0) on the slow channels (relu of a block output is itself) and the fusion BatchNorm on the tail.
The backward walks the saved records in reverse.  No entry point issues an atomic: training steps are bit-reproducible.
"""
import ctypes as C

import torch

from . import lib as L
from . import plans
from . import slowfast as S


class Fm:
    """A feature map: t is a [N*T*H*W, C] view (row pitch t.stride(0)) over the grid (N, T, H, W)."""
    __slots__ = ("t", "N", "T", "H", "W")

    def __init__(self, t, N, T, H, W):
        assert t.dim() == 2 and t.stride(1) == 1 and t.shape[0] == N * T * H * W, (tuple(t.shape), N, T, H, W)
        self.t, self.N, self.T, self.H, self.W = t, N, T, H, W

    @property
    def C(self):
        return self.t.shape[1]

    @property
    def ld(self):
        return self.t.stride(0)

    @property
    def rows(self):
        return self.t.shape[0]


def _desc(x, k, s, p, cout, ldy):
    kt, kh, kw = k
    To, Ho, Wo = [(n + 2 * pp - kk) // ss + 1 for n, kk, ss, pp in zip((x.T, x.H, x.W), k, s, p)]
    d = L.Conv3dDesc(N=x.N, T=x.T, H=x.H, W=x.W, C=x.C, To=To, Ho=Ho, Wo=Wo, K=cout, kt=kt, kh=kh, kw=kw, st=s[0], sh=s[1], sw=s[2],
                     pt=p[0], ph=p[1], pw=p[2], ldx=x.ld, ldy=ldy)
    return d, (To, Ho, Wo)


def _pack_w(w, cin):
    """torch weight [K, C, kt, kh, kw] -> [K, kt*kh*kw*cin] (cin >= C: zero input channels appended, the stems' 4th channel)."""
    wp = w.detach().permute(0, 2, 3, 4, 1)
    if cin != w.shape[1]:
        wp = torch.nn.functional.pad(wp, (0, cin - w.shape[1]))
    return wp.reshape(w.shape[0], -1).contiguous()


def _pack_wt(w):
    """torch weight [K, C, kt, kh, kw] -> [kt*kh*kw*K, C] (the data gradient's operand)."""
    return w.detach().permute(2, 3, 4, 0, 1).reshape(-1, w.shape[1]).contiguous()


class Conv:
    def __init__(self, key, k, s, p):
        self.key, self.k, self.s, self.p = key, tuple(k), tuple(s), tuple(p)


def conv_fwd(x, w, conv, pro, out=None, stats=True):
    """z = conv(pro(x)); returns (Fm z, fp64 stats [2][K] or None)."""
    cout = w.shape[0]
    lib = L.get()
    d, (To, Ho, Wo) = _desc(x, conv.k, conv.s, conv.p, cout, out.stride(0) if out is not None else cout)
    rows = x.N * To * Ho * Wo
    if out is None:
        out = torch.empty(rows, cout, dtype=torch.float32, device=x.t.device)
    wp = _pack_w(w, x.C)
    st = part = None
    if stats:
        part = torch.empty(int(lib.mt_conv3d_part_floats(C.byref(d))), dtype=torch.float32, device=out.device)
        st = torch.empty(2 * cout, dtype=torch.float64, device=out.device)
    sc, sh = pro if pro is not None else (None, None)
    L.mt.conv3d_fwd(d, x.t, sc, sh, wp, out, 0, part, st)
    return Fm(out, x.N, To, Ho, Wo), st


def conv_wgrad(x, pro, dz, w, conv):
    """dW of conv (torch layout) from the input x (with its prologue) and dz = dL/dz."""
    lib = L.get()
    d, _ = _desc(x, conv.k, conv.s, conv.p, w.shape[0], dz.ld)
    splits = int(lib.mt_conv3d_wgrad_splits(C.byref(d)))
    kd = conv.k[0] * conv.k[1] * conv.k[2] * x.C
    dwp = torch.empty(w.shape[0], kd, dtype=torch.float32, device=dz.t.device)
    ws = torch.empty(splits * w.shape[0] * kd, dtype=torch.float32, device=dz.t.device) if splits > 1 else None
    sc, sh = pro if pro is not None else (None, None)
    L.mt.conv3d_wgrad(d, x.t, sc, sh, dz.t, dwp, ws, splits)
    kt, kh, kw = conv.k
    g = dwp.reshape(w.shape[0], kt, kh, kw, x.C)[..., :w.shape[1]]
    return g.permute(0, 4, 1, 2, 3).contiguous()


def conv_dgrad(x, dz, w, conv, out, accumulate):
    """out (+)= d conv / d pro(x) applied to dz; out is a [rows_x, C] tensor (any pitch)."""
    d, _ = _desc(Fm(out, x.N, x.T, x.H, x.W), conv.k, conv.s, conv.p, w.shape[0], dz.ld)
    L.mt.conv3d_dgrad(d, dz.t, _pack_wt(w), out, int(accumulate))


def _pack_w_stem_dgrad(w):
    """torch stem weight [K, 3, kt, 7, 7] -> [kt*K, 160]: row dt*K + co, column (kh*7 + kw)*3 + c, columns 147..159 zero (the operand
    of mt_sf_stem_dgrad)."""
    wt = w.detach().permute(2, 0, 3, 4, 1).reshape(w.shape[2] * w.shape[0], -1)
    return torch.nn.functional.pad(wt, (0, 160 - wt.shape[1])).contiguous()


def stem_dgrad(x, dz, w):
    """The stem's data gradient down to the packed clip: dz = dL/dz of the stem convolution of x -> dL/dx as [N, T, H, W, 4]."""
    dx = torch.empty(x.N, x.T, x.H, x.W, 4, dtype=torch.float32, device=dz.t.device)
    L.mt.sf_stem_dgrad(dz.t, dz.ld, _pack_w_stem_dgrad(w), dx, x.N, x.T, x.H, x.W, w.shape[2], w.shape[0])
    return dx


class BN:
    """Folded BatchNorm of one layer: scale, shift, mean_invstd."""
    __slots__ = ("key", "scale", "shift", "mi", "count", "training")


def bn_fwd(ctx, key, stats, count):
    mod = ctx.bn_mods[key]
    gamma, beta = ctx.P[key + ".weight"], ctx.P[key + ".bias"]
    Cn = gamma.shape[0]
    dev = gamma.device
    b = BN()
    b.key, b.count, b.training = key, count, ctx.training
    b.scale = torch.empty(Cn, dtype=torch.float32, device=dev)
    b.shift = torch.empty(Cn, dtype=torch.float32, device=dev)
    b.mi = torch.empty(2 * Cn, dtype=torch.float32, device=dev)
    if ctx.training and mod.momentum is None:
        raise NotImplementedError("SlowFast: BatchNorm momentum None (cumulative average) is not supported")
    L.mt.bn_finalize(stats if ctx.training else None, 1, float(count), gamma, beta, mod.running_mean, mod.running_var, b.scale, b.shift,
                     b.mi, Cn, float(mod.eps), float(mod.momentum or 0.0), int(ctx.training))
    if ctx.training and mod.num_batches_tracked is not None:
        mod.num_batches_tracked.add_(1)
    return b


def bn_bwd(ctx, b, g, z, relu_bn=None, mask=None, out=None, accumulate=False):
    """BatchNorm(+ReLU) adjoint: returns dz = dL/dz ([rows, C] tensor: out or new) from g = dL/d(output).  The ReLU mask is
    relu_bn's (z * scale + shift > 0) or (mask > 0).  Accumulates dgamma / dbeta into ctx.grads."""
    lib = L.get()
    rows, Cn = z.t.shape
    dev = z.t.device
    sc, sh = (relu_bn.scale, relu_bn.shift) if relu_bn is not None else (None, None)
    mt, ldm = (mask.t, mask.ld) if mask is not None else (None, 0)
    part = torch.empty(int(lib.mt_sf_bn_bwd_part_floats(rows, Cn)), dtype=torch.float32, device=dev)
    st = torch.empty(2 * Cn, dtype=torch.float64, device=dev)
    L.mt.sf_bn_relu_bwd_stats(g.t, g.ld, z.t, z.ld, sc, sh, mt, ldm, b.mi, part, st, rows, Cn)
    kabc = torch.empty(3 * Cn, dtype=torch.float32, device=dev)
    dgamma, dbeta = ctx.grad_buf(b.key + ".weight"), ctx.grad_buf(b.key + ".bias")
    L.mt.bn_bwd_finalize(st, 1, float(b.count), ctx.P[b.key + ".weight"], b.mi, kabc, dgamma, dbeta, Cn, int(b.training))
    if out is None:
        out = torch.empty(rows, Cn, dtype=torch.float32, device=dev)
    L.mt.sf_bn_relu_bwd_apply(g.t, g.ld, z.t, z.ld, sc, sh, mt, ldm, kabc, out, out.stride(0), int(accumulate), rows, Cn)
    return Fm(out, z.N, z.T, z.H, z.W)


def _block_keys(prefix, first):
    k = {n: f"{prefix}.branch2.{n}" for n in ("conv_a", "norm_a", "conv_b", "norm_b", "conv_c", "norm_c")}
    if first:
        k["branch1_conv"], k["branch1_norm"] = f"{prefix}.branch1_conv", f"{prefix}.branch1_norm"
    return k


class Rec:
    """What one bottleneck's backward needs."""
    pass


def block_fwd(ctx, prefix, x, pro, kt, stride, first, out=None):
    keys = _block_keys(prefix, first)
    P = ctx.P
    ca = Conv(keys["conv_a"], (kt, 1, 1), (1, 1, 1), (kt // 2, 0, 0))
    cb = Conv(keys["conv_b"], (1, 3, 3), (1, stride, stride), (0, 1, 1))
    cc = Conv(keys["conv_c"], (1, 1, 1), (1, 1, 1), (0, 0, 0))
    za, sa = conv_fwd(x, P[ca.key + ".weight"], ca, pro, stats=ctx.training)
    ba = bn_fwd(ctx, keys["norm_a"], sa, za.rows)
    zb, sb = conv_fwd(za, P[cb.key + ".weight"], cb, (ba.scale, ba.shift), stats=ctx.training)
    bb = bn_fwd(ctx, keys["norm_b"], sb, zb.rows)
    zc, scs = conv_fwd(zb, P[cc.key + ".weight"], cc, (bb.scale, bb.shift), stats=ctx.training)
    bc = bn_fwd(ctx, keys["norm_c"], scs, zc.rows)
    r = Rec()
    r.z1 = r.b1 = r.c1 = None
    if first:
        c1 = Conv(keys["branch1_conv"], (1, 1, 1), (1, stride, stride), (0, 0, 0))
        z1, s1 = conv_fwd(x, P[c1.key + ".weight"], c1, pro, stats=ctx.training)
        b1 = bn_fwd(ctx, keys["branch1_norm"], s1, z1.rows)
        res, ldr, rsc, rsh = z1.t, z1.ld, b1.scale, b1.shift
        r.z1, r.b1, r.c1 = z1, b1, c1
    else:
        assert pro is None and x.C == zc.C
        res, ldr, rsc, rsh = x.t, x.ld, None, None
    if out is None:
        out = torch.empty(zc.rows, zc.C, dtype=torch.float32, device=zc.t.device)
    L.mt.sf_bn_relu_fwd(zc.t, zc.ld, bc.scale, bc.shift, res, ldr, rsc, rsh, out, out.stride(0), zc.rows, zc.C)
    y = Fm(out, zc.N, zc.T, zc.H, zc.W)
    r.x, r.pro, r.za, r.zb, r.zc, r.ba, r.bb, r.bc, r.ca, r.cb, r.cc, r.y = x, pro, za, zb, zc, ba, bb, bc, ca, cb, cc, y
    return y, r


def block_bwd(ctx, r, gy):
    """gy = dL/dy (Fm, any pitch) -> dL/d pro(x) as a new [rows_x, C_x] tensor."""
    P = ctx.P
    dev = gy.t.device
    gx = torch.empty(r.x.rows, r.x.C, dtype=torch.float32, device=dev)
    dzc = bn_bwd(ctx, r.bc, gy, r.zc, mask=r.y)
    if r.z1 is not None:
        dz1 = bn_bwd(ctx, r.b1, gy, r.z1, mask=r.y)
        ctx.add_wgrad(r.c1.key, r.x, r.pro, dz1, r.c1)
        conv_dgrad(r.x, dz1, P[r.c1.key + ".weight"], r.c1, gx, False)
    else:
        L.mt.sf_bn_relu_bwd_apply(gy.t, gy.ld, None, 0, None, None, r.y.t, r.y.ld, None, gx, gx.stride(0), 0, r.y.rows, r.y.C)
    ctx.add_wgrad(r.cc.key, r.zb, (r.bb.scale, r.bb.shift), dzc, r.cc)
    gb = torch.empty(r.zb.rows, r.zb.C, dtype=torch.float32, device=dev)
    conv_dgrad(r.zb, dzc, P[r.cc.key + ".weight"], r.cc, gb, False)
    del dzc
    dzb = bn_bwd(ctx, r.bb, Fm(gb, r.zb.N, r.zb.T, r.zb.H, r.zb.W), r.zb, relu_bn=r.bb, out=gb)
    ctx.add_wgrad(r.cb.key, r.za, (r.ba.scale, r.ba.shift), dzb, r.cb)
    ga = torch.empty(r.za.rows, r.za.C, dtype=torch.float32, device=dev)
    conv_dgrad(r.za, dzb, P[r.cb.key + ".weight"], r.cb, ga, False)
    del dzb, gb
    dza = bn_bwd(ctx, r.ba, Fm(ga, r.za.N, r.za.T, r.za.H, r.za.W), r.za, relu_bn=r.ba, out=ga)
    ctx.add_wgrad(r.ca.key, r.x, r.pro, dza, r.ca)
    conv_dgrad(r.x, dza, P[r.ca.key + ".weight"], r.ca, gx, True)
    return gx


class _Walk:
    """State of one forward / backward: parameters by name, BatchNorm modules, gradient buffers."""

    def __init__(self, model, names, params, training):
        self.P = dict(zip(names, params))
        self.names = names
        self.training = training
        self.bn_mods = {n: m for n, m in model.named_modules() if isinstance(m, torch.nn.BatchNorm3d)}
        self.grads = {}
        self.need = {}

    def grad_buf(self, key):
        g = self.grads.get(key)
        if g is None:
            g = self.grads[key] = torch.zeros_like(self.P[key])
        return g

    def add_wgrad(self, key, x, pro, dz, conv):
        if self.need.get(key + ".weight", True):
            self.grads[key + ".weight"] = conv_wgrad(x, pro, dz, self.P[key + ".weight"], conv)


def _fusion_fwd(ctx, key, xf, cat, cs):
    """Fusion conv of the fast map xf written raw into cat[:, cs:]; returns the prologue (scale, shift) over all of cat's channels."""
    conv = Conv(key + ".conv_fast_to_slow", (S.FUSION_KERNEL, 1, 1), (S.FUSION_STRIDE, 1, 1), (S.FUSION_KERNEL // 2, 0, 0))
    z, st = conv_fwd(xf, ctx.P[conv.key + ".weight"], conv, None, out=cat[:, cs:], stats=ctx.training)
    b = bn_fwd(ctx, key + ".norm", st, z.rows)
    dev = cat.device
    scale = torch.cat([torch.ones(cs, device=dev), b.scale])
    shift = torch.cat([torch.zeros(cs, device=dev), b.shift])
    return (scale, shift), (conv, z, b, xf)


def _fusion_bwd(ctx, rec, gcat, cs, gxf):
    """gcat = dL/d pro(cat): the fusion tail's adjoint; adds the fast map's gradient into gxf."""
    conv, z, b, xf = rec
    g = Fm(gcat[:, cs:], z.N, z.T, z.H, z.W)
    dz = bn_bwd(ctx, b, g, z, relu_bn=b)
    ctx.add_wgrad(conv.key, xf, None, dz, conv)
    conv_dgrad(xf, dz, ctx.P[conv.key + ".weight"], conv, gxf, True)


def _stem_fwd(ctx, key, x, kt, out):
    conv = Conv(key + ".conv", (kt, 7, 7), (1, 2, 2), (kt // 2, 3, 3))
    z, st = conv_fwd(x, ctx.P[conv.key + ".weight"], conv, None, stats=ctx.training)
    b = bn_fwd(ctx, key + ".norm", st, z.rows)
    Ho, Wo = (z.H - 1) // 2 + 1, (z.W - 1) // 2 + 1
    rows = z.N * z.T * Ho * Wo
    if out is None:
        out = torch.empty(rows, z.C, dtype=torch.float32, device=z.t.device)
    arg = torch.empty(rows, z.C, dtype=torch.int32, device=z.t.device)
    L.mt.sf_maxpool_fwd(z.t, b.scale, b.shift, out, out.stride(0), arg, z.N * z.T, z.H, z.W, z.C)
    return Fm(out, z.N, z.T, Ho, Wo), (conv, x, z, b, arg)


def _stem_bwd(ctx, rec, gp, want_dx=False):
    """Adjoint of the stem from gp = dL/d(pool output); want_dx: also returns dL/d(clip) as a packed [N, T, H, W, 4] tensor."""
    conv, x, z, b, arg = rec
    din = torch.empty(z.rows, z.C, dtype=torch.float32, device=z.t.device)
    L.mt.sf_maxpool_bwd(gp.t, gp.ld, arg, din, z.N * z.T, z.H, z.W, z.C)
    dz = bn_bwd(ctx, b, Fm(din, z.N, z.T, z.H, z.W), z, relu_bn=b, out=din)
    ctx.add_wgrad(conv.key, x, None, dz, conv)
    return stem_dgrad(x, dz, ctx.P[conv.key + ".weight"]) if want_dx else None


def _dropout_mult(model, B, P, dev):
    head = model.blocks[6]
    p = float(head.dropout.p)
    if not (head.dropout.training and p > 0.0):
        return None
    Pt, Ph, Pw = P
    shape = (B, S.HEAD_DIM, Pt, Ph, Pw)
    sampler = getattr(model, "dropout_uniform", None)
    u = sampler(shape, dev) if sampler is not None else torch.rand(shape, device=dev, dtype=torch.float32)
    mult = (u.to(device=dev, dtype=torch.float32) >= p).float() / (1.0 - p)
    return mult.permute(0, 2, 3, 4, 1).reshape(B, Pt * Ph * Pw, S.HEAD_DIM).contiguous()


def network_forward(ctx, model, xs, xf):
    """The layer walk; returns (logits, records)."""
    P = ctx.P
    cs0, cf0 = S.STEM_OUT
    dev = xs.t.device
    cat_w = cs0 + S.FUSION_RATIO * cf0
    Hs, Ws = (xs.H - 1) // 2 + 1, (xs.W - 1) // 2 + 1
    Hp, Wp = (Hs - 1) // 2 + 1, (Ws - 1) // 2 + 1
    cat = torch.empty(xs.N * xs.T * Hp * Wp, cat_w, dtype=torch.float32, device=dev)
    ps, rs_stem = _stem_fwd(ctx, "blocks.0.multipathway_blocks.0", xs, 1, cat[:, :cs0])
    pf, rf_stem = _stem_fwd(ctx, "blocks.0.multipathway_blocks.1", xf, 5, None)
    pro, rfus = _fusion_fwd(ctx, "blocks.0.multipathway_fusion", pf, cat, cs0)
    recs = {"stem": (rs_stem, rf_stem, rfus, ps)}
    xsl = Fm(cat, ps.N, ps.T, ps.H, ps.W)
    xfa = pf
    stages = []
    for s in range(4):
        depth = S.DEPTHS[s]
        last_fusion = s < 3
        sl, fa = [], []
        for i in range(depth):          # fast pathway first: the fusion reads its output
            yfa, r = block_fwd(ctx, f"blocks.{s + 1}.multipathway_blocks.1.res_blocks.{i}", xfa, None, S.FAST_CONV_A_T[s],
                               S.STAGE_STRIDE[s] if i == 0 else 1, i == 0)
            fa.append(r)
            xfa = yfa
        pro_s = pro
        cat_next = None
        for i in range(depth):
            out = None
            if i == depth - 1 and last_fusion:
                # the last slow block writes into the head of the concatenated tensor; the fusion fills its tail
                cat_next = torch.empty(yfa.rows // S.ALPHA, S.SLOW_OUT[s] + S.FUSION_RATIO * S.FAST_OUT[s], dtype=torch.float32,
                                       device=dev)
                out = cat_next[:, :S.SLOW_OUT[s]]
            ysl, r = block_fwd(ctx, f"blocks.{s + 1}.multipathway_blocks.0.res_blocks.{i}", xsl, pro_s, S.SLOW_CONV_A_T[s],
                               S.STAGE_STRIDE[s] if i == 0 else 1, i == 0, out=out)
            sl.append(r)
            xsl, pro_s = ysl, None
        fus = None
        if last_fusion:
            pro, fus = _fusion_fwd(ctx, f"blocks.{s + 1}.multipathway_fusion", yfa, cat_next, S.SLOW_OUT[s])
            xsl = Fm(cat_next, ysl.N, ysl.T, ysl.H, ysl.W)
        stages.append((sl, fa, fus))
    recs["stages"] = stages
    # head
    B = xs.N
    (kts, khs, kws), (ktf, khf, kwf) = model.head_pool_kernel_sizes
    Pdims = (xsl.T - kts + 1, xsl.H - khs + 1, xsl.W - kws + 1)
    if Pdims != (xfa.T - ktf + 1, xfa.H - khf + 1, xfa.W - kwf + 1) or min(Pdims) < 1:
        raise ValueError(f"SlowFast head: the pooled grids of the two pathways differ or are empty (slow {(xsl.T, xsl.H, xsl.W)} with "
                         f"kernel {(kts, khs, kws)}, fast {(xfa.T, xfa.H, xfa.W)} with {(ktf, khf, kwf)})")
    Pn = Pdims[0] * Pdims[1] * Pdims[2]
    mult = _dropout_mult(model, B, Pdims, dev)
    d = torch.empty(B, Pn, S.HEAD_DIM, dtype=torch.float32, device=dev)
    for feat, (kt, kh, kw), coff in ((xsl, (kts, khs, kws), 0), (xfa, (ktf, khf, kwf), S.SLOW_OUT[-1])):
        L.mt.sf_head_pool(feat.t, feat.ld, mult, d, B, feat.T, feat.H, feat.W, feat.C, kt, kh, kw, coff, S.HEAD_DIM)
    w, bias = P["proj.weight"], P["proj.bias"]
    J = w.shape[0]
    logits = torch.empty(B, J, dtype=torch.float32, device=dev)
    L.mt.sf_head_proj(d, w, bias, logits, B, Pn, S.HEAD_DIM, J)
    recs["head"] = (xsl, xfa, d, mult, Pn, ((kts, khs, kws), (ktf, khf, kwf)))
    return logits, recs


def network_backward(ctx, recs, g, need_x=(False, False)):
    """The reverse walk; need_x: return dL/d(packed slow clip), dL/d(packed fast clip) where asked for (else None)."""
    dev = g.device
    xsl, xfa, d, mult, Pn, ((kts, khs, kws), (ktf, khf, kwf)) = recs["head"]
    B, J = g.shape
    w = ctx.P["proj.weight"]
    dpool = torch.empty(B, Pn, S.HEAD_DIM, dtype=torch.float32, device=dev)
    dw = ctx.grad_buf("proj.weight")
    db = ctx.grad_buf("proj.bias") if "proj.bias" in ctx.P else None
    L.mt.sf_head_bwd(g, d, w, mult, dw, db, dpool, B, Pn, S.HEAD_DIM, J)
    gs = torch.empty(xsl.rows, xsl.C, dtype=torch.float32, device=dev)
    gf = torch.empty(xfa.rows, xfa.C, dtype=torch.float32, device=dev)
    for feat, gt, (kt, kh, kw), coff in ((xsl, gs, (kts, khs, kws), 0), (xfa, gf, (ktf, khf, kwf), S.SLOW_OUT[-1])):
        L.mt.sf_head_dfeat(dpool, gt, gt.stride(0), B, feat.T, feat.H, feat.W, feat.C, kt, kh, kw, coff, S.HEAD_DIM)
    gsl = Fm(gs, xsl.N, xsl.T, xsl.H, xsl.W)
    gfa = Fm(gf, xfa.N, xfa.T, xfa.H, xfa.W)
    for s in reversed(range(4)):
        sl, fa, fus = recs["stages"][s]
        if fus is not None:
            # gsl is dL/d pro(cat) of the next stage's input: slow head = dL/d y_slow, fusion tail -> fast output
            _fusion_bwd(ctx, fus, gsl.t, S.SLOW_OUT[s], gfa.t)
            gsl = Fm(gsl.t[:, :S.SLOW_OUT[s]], gsl.N, gsl.T, gsl.H, gsl.W)
        for r in reversed(sl):
            gx = block_bwd(ctx, r, gsl)
            gsl = Fm(gx, r.x.N, r.x.T, r.x.H, r.x.W)
        for r in reversed(fa):
            gx = block_bwd(ctx, r, gfa)
            gfa = Fm(gx, r.x.N, r.x.T, r.x.H, r.x.W)
    rs_stem, rf_stem, rfus, ps = recs["stem"]
    _fusion_bwd(ctx, rfus, gsl.t, S.STEM_OUT[0], gfa.t)
    dxs = _stem_bwd(ctx, rs_stem, Fm(gsl.t[:, :S.STEM_OUT[0]], gsl.N, gsl.T, gsl.H, gsl.W), need_x[0])
    dxf = _stem_bwd(ctx, rf_stem, gfa, need_x[1])
    return dxs, dxf


class _SlowFastFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, mode, xs_buf, xf_buf, *params):
        grad_on, names, training = mode
        save = grad_on and any(ctx.needs_input_grad[2:])
        walk = _Walk(model, names, params, training)
        B, Ts, H, W, _ = xs_buf.shape
        Tf = xf_buf.shape[1]
        xs = Fm(xs_buf.view(-1, 4), B, Ts, H, W)
        xf = Fm(xf_buf.view(-1, 4), xf_buf.shape[0], Tf, xf_buf.shape[2], xf_buf.shape[3])
        logits, recs = network_forward(walk, model, xs, xf)
        ctx.walk = walk
        ctx.recs = recs if save else None
        ctx.stamp = plans.stamp(params) if save else None
        ctx.params = params
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        if ctx.recs is None:
            plans.refuse_second_pass("SlowFast")
        plans.check_stamp(ctx.params, ctx.stamp, "SlowFast", "the parameters")
        walk = ctx.walk
        need = ctx.needs_input_grad[4:]
        walk.need = {n: bool(r) for n, r in zip(walk.names, need)}
        dxs, dxf = network_backward(walk, ctx.recs, dlogits.contiguous().float(), ctx.needs_input_grad[2:4])
        ctx.recs = None
        out = []
        for n, r in zip(walk.names, need):
            out.append(walk.grads.get(n) if r else None)
        return (None, None, dxs, dxf, *out)


def _named_params(model):
    """(names, tensors) of every parameter in walk naming: the network's by state-dict name, the head's Linear as proj.* (read from
    blocks[6].proj at call time)."""
    names, ps = [], []
    for n, p in model.named_parameters():
        if n.startswith("blocks.6.proj."):
            continue
        names.append(n)
        ps.append(p)
    proj = model.blocks[6].proj
    names.append("proj.weight")
    ps.append(proj.weight)
    if proj.bias is not None:
        names.append("proj.bias")
        ps.append(proj.bias)
    return names, ps


def slowfast_apply(model, x):
    if not isinstance(x, (list, tuple)) or len(x) != 2:
        raise ValueError("SlowFast expects [slow, fast] pathway inputs ([B, 3, T, H, W] each), as PackPathway returns")
    xs_buf = S.pack_pathway_input(x[0])
    xf_buf = S.pack_pathway_input(x[1])
    if xs_buf.shape[0] != xf_buf.shape[0] or xs_buf.shape[2:4] != xf_buf.shape[2:4] or xf_buf.shape[1] != S.ALPHA * xs_buf.shape[1]:
        raise ValueError(f"SlowFast: slow {tuple(xs_buf.shape)} and fast {tuple(xf_buf.shape)} pathways do not pair (alpha {S.ALPHA})")
    names, params = _named_params(model)
    proj = model.blocks[6].proj
    if not isinstance(proj, torch.nn.Linear) or proj.in_features != S.HEAD_DIM:
        raise ValueError(f"SlowFast: blocks[6].proj must be an nn.Linear({S.HEAD_DIM}, k)")
    if any(not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous() for p in params):
        raise L.MintimeHipError("SlowFast: parameters must be contiguous fp32 device tensors (call .cuda())")
    training = model.training
    return _SlowFastFunction.apply(model, (torch.is_grad_enabled(), tuple(names), training), xs_buf, xf_buf, *params)
