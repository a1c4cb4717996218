"""The launch sequence of the FaceNet InceptionResnetV1 embedder (facenet.py) on csrc/facenet.hip.  Inference only.

  * Every BatchNorm folds into its convolution once (`fold_conv_bn`: w' = w g / sqrt(var + eps), b' = beta - mean g / sqrt(var + eps),
    computed in fp64), `last_bn` into `last_linear` the same way.  The folded weights are repacked to [K][kh][kw][C] (the stem's 3
    input channels padded to 4) and kept under `plans.stamp(...)` of the module's tensors: a load_state_dict, an in-place edit or a
    move of the module refolds them, into the same storage.
  * Activations are channels-last rows with a row pitch.  A branch's last convolution writes its channel slice of the concatenation
    buffer, and so do the max-pool branches of mixed_6a / mixed_7a: there is no cat launch.
  * Sibling 1 x 1 convolutions of one input run as one launch with their output channels side by side: branch1.0 + branch2.0 of
    Block35 (64 channels), branch0 + branch1.0 of Block17 and Block8 (written straight into the concatenation buffer, whose second
    half the branch's last convolution later overwrites), the three 896 -> 256 of mixed_7a.  109 convolution launches instead of 132.
  * A batch runs in chunks of `chunk` faces over one arena per (H, W); the launch list of a (faces, H, W) is built once.  After the
    first call at a shape nothing is allocated and nothing is read back.
"""
import ctypes as C
from collections import namedtuple

import torch

from . import lib as L
from . import plans

MIN_SIDE = 75
CHUNK = 256
BN_EPS = 1e-3
NORM_EPS = 1e-12


def stage_sizes(n):
    """Side lengths along one axis after conv2d_1a, 2a, 2b, maxpool_3a, 3b, 4a, 4b, mixed_6a, mixed_7a."""
    s = [(n - 3) // 2 + 1]
    s.append(s[-1] - 2)
    s.append(s[-1])
    s.append((s[-1] - 3) // 2 + 1)
    s.append(s[-1])
    s.append(s[-1] - 2)
    s.append((s[-1] - 3) // 2 + 1)
    s.append((s[-1] - 3) // 2 + 1)
    s.append((s[-1] - 3) // 2 + 1)
    return s


def check_side(H, W):
    if H < MIN_SIDE or W < MIN_SIDE:
        raise ValueError(f"InceptionResnetV1: {H} x {W} faces are too small, the smallest input is {MIN_SIDE} x {MIN_SIDE} "
                         "(mixed_7a needs a 3 x 3 grid)")


def fold_conv_bn(w, gamma, beta, mean, var, eps=BN_EPS, bias=None):
    """(w', b') with conv(x, w') + b' == bn(conv(x, w) + bias) in eval mode; computed in fp64, returned in w's dtype.
    w: [K, ...]; gamma, beta, mean, var: [K]."""
    s = gamma.double() / torch.sqrt(var.double() + eps)
    wf = w.double() * s.reshape(-1, *([1] * (w.dim() - 1)))
    b0 = mean.double() if bias is None else mean.double() - bias.double()
    bf = beta.double() - b0 * s
    return wf.to(w.dtype), bf.to(w.dtype)


def pack_weight(w):
    """torch conv weight [K, C, kh, kw] -> [K][kh][kw][C4] contiguous, C padded with zeros to a multiple of 4."""
    K, Cc, kh, kw = w.shape
    p = w.permute(0, 2, 3, 1)
    if Cc % 4:
        p = torch.nn.functional.pad(p, (0, 4 - Cc % 4))
    return p.contiguous()


class View(namedtuple("View", "buf off C ld h w")):
    """`C` channels starting at column `off` of the rows of arena buffer `buf` (pitch `ld`), an h x w grid per face."""

    def slice(self, off, C_):
        return View(self.buf, self.off + off, C_, self.ld, self.h, self.w)


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


class _Builder:
    """Collects the operations of one (N, H, W) and the floats each arena buffer needs."""

    def __init__(self, engine, N, H, W):
        self.e, self.N, self.H, self.W = engine, N, H, W
        self.ops, self.need = [], {}

    def _claim(self, buf, rows, ld):
        self.need[buf] = max(self.need.get(buf, 0), rows * ld)

    def ingest(self):
        self._claim("in4", self.N * self.H * self.W, 4)
        return View("in4", 0, 4, 4, self.H, self.W)

    def conv(self, unit, x, dst, k=1, s=1, p=0, act=1, res=None, scale=1.0):
        (kh, kw), (sh, sw), (ph, pw) = _pair(k), _pair(s), _pair(p)
        K, Cw, wkh, wkw = self.e.unit_shape(unit)
        assert (Cw, wkh, wkw) == (x.C, kh, kw), (unit, x, k)
        ho, wo = (x.h + 2 * ph - kh) // sh + 1, (x.w + 2 * pw - kw) // sw + 1
        buf, off, ld = dst
        assert buf != x.buf and (res is None or buf != res.buf) and off + K <= ld and off % 4 == 0 and x.off % 4 == 0
        d = L.Conv2dDesc()
        d.N, d.H, d.W, d.C, d.Ho, d.Wo, d.K = self.N, x.h, x.w, x.C, ho, wo, K
        d.kh, d.kw, d.sh, d.sw, d.ph, d.pw, d.act, d.res_scale = kh, kw, sh, sw, ph, pw, int(act), float(scale)
        d.ldx, d.ldy, d.ldr = x.ld, ld, (res.ld if res is not None else 0)
        if res is not None:
            assert (res.C, res.h, res.w) == (K, ho, wo)
        self._claim(buf, self.N * ho * wo, ld)
        self.ops.append(("conv", d, unit, x, (buf, off), res))
        return View(buf, off, K, ld, ho, wo)

    def maxpool(self, x, dst):
        buf, off, ld = dst
        ho, wo = (x.h - 3) // 2 + 1, (x.w - 3) // 2 + 1
        assert buf != x.buf and off + x.C <= ld and off % 4 == 0
        self._claim(buf, self.N * ho * wo, ld)
        self.ops.append(("maxpool", x, (buf, off, ld)))
        return View(buf, off, x.C, ld, ho, wo)

    def avgpool(self, x, dst):
        buf, off, ld = dst
        self._claim(buf, self.N, ld)
        self.ops.append(("avgpool", x, (buf, off, ld)))
        return View(buf, off, x.C, ld, 1, 1)


def _other(x):
    return "B" if x.buf == "A" else "A"


def _program(b, m):
    """The network as launches; `m` is the InceptionResnetV1 module (its submodules name the weights)."""
    e = b.e
    u, plain = e.unit_bc, e.unit_plain
    x = b.ingest()
    x = b.conv(u(m.conv2d_1a), x, ("A", 0, 32), 3, 2)
    x = b.conv(u(m.conv2d_2a), x, ("B", 0, 32), 3)
    x = b.conv(u(m.conv2d_2b), x, ("A", 0, 64), 3, 1, 1)
    x = b.maxpool(x, ("B", 0, 64))
    x = b.conv(u(m.conv2d_3b), x, ("A", 0, 80), 1)
    x = b.conv(u(m.conv2d_4a), x, ("B", 0, 192), 3)
    x = b.conv(u(m.conv2d_4b), x, ("A", 0, 256), 3, 2)
    for blk in m.repeat_1:                                                   # Block35
        b.conv(u(blk.branch0), x, ("cat", 0, 96))
        t = b.conv(u(blk.branch1[0], blk.branch2[0]), x, ("t0", 0, 64))
        b.conv(u(blk.branch1[1]), t.slice(0, 32), ("cat", 32, 96), 3, 1, 1)
        t = b.conv(u(blk.branch2[1]), t.slice(32, 32), ("t1", 0, 32), 3, 1, 1)
        b.conv(u(blk.branch2[2]), t, ("cat", 64, 96), 3, 1, 1)
        x = b.conv(plain(blk.conv2d), View("cat", 0, 96, 96, x.h, x.w), (_other(x), 0, 256), res=x, scale=blk.scale)
    o = _other(x)                                                            # mixed_6a
    y = b.conv(u(m.mixed_6a.branch0), x, (o, 0, 896), 3, 2)
    t = b.conv(u(m.mixed_6a.branch1[0]), x, ("t0", 0, 192))
    t = b.conv(u(m.mixed_6a.branch1[1]), t, ("t1", 0, 192), 3, 1, 1)
    b.conv(u(m.mixed_6a.branch1[2]), t, (o, 384, 896), 3, 2)
    b.maxpool(x, (o, 640, 896))
    x = View(o, 0, 896, 896, y.h, y.w)
    for blk in m.repeat_2:                                                   # Block17
        cat = b.conv(u(blk.branch0, blk.branch1[0]), x, ("cat", 0, 256))
        t = b.conv(u(blk.branch1[1]), cat.slice(128, 128), ("t1", 0, 128), (1, 7), 1, (0, 3))
        b.conv(u(blk.branch1[2]), t, ("cat", 128, 256), (7, 1), 1, (3, 0))
        x = b.conv(plain(blk.conv2d), cat, (_other(x), 0, 896), res=x, scale=blk.scale)
    o = _other(x)                                                            # mixed_7a
    t = b.conv(u(m.mixed_7a.branch0[0], m.mixed_7a.branch1[0], m.mixed_7a.branch2[0]), x, ("t0", 0, 768))
    y = b.conv(u(m.mixed_7a.branch0[1]), t.slice(0, 256), (o, 0, 1792), 3, 2)
    b.conv(u(m.mixed_7a.branch1[1]), t.slice(256, 256), (o, 384, 1792), 3, 2)
    t = b.conv(u(m.mixed_7a.branch2[1]), t.slice(512, 256), ("t1", 0, 256), 3, 1, 1)
    b.conv(u(m.mixed_7a.branch2[2]), t, (o, 640, 1792), 3, 2)
    b.maxpool(x, (o, 896, 1792))
    x = View(o, 0, 1792, 1792, y.h, y.w)
    for blk in list(m.repeat_3) + [m.block8]:                                # Block8
        cat = b.conv(u(blk.branch0, blk.branch1[0]), x, ("cat", 0, 384))
        t = b.conv(u(blk.branch1[1]), cat.slice(192, 192), ("t1", 0, 192), (1, 3), 1, (0, 1))
        b.conv(u(blk.branch1[2]), t, ("cat", 192, 384), (3, 1), 1, (1, 0))
        x = b.conv(plain(blk.conv2d), cat, (_other(x), 0, 1792), act=0 if blk.noReLU else 1, res=x, scale=blk.scale)
    x = b.avgpool(x, ("pool", 0, 1792))
    return b.conv(e.unit_linear(m.last_linear, m.last_bn), x, ("lin", 0, 512), act=0)


class Engine:
    def __init__(self, model):
        self.model = model
        self.units, self.index = [], {}           # unit = ("bc", BasicConv2d...) | ("plain", Conv2d) | ("linear", Linear, BatchNorm1d)
        self.folded, self.stamp = None, None
        self.arenas, self.programs, self.outs = {}, {}, {}
        self.chunk = CHUNK
        _program(_Builder(self, 1, MIN_SIDE, MIN_SIDE), model)        # registers every weight unit

    # ---- weights
    def _unit(self, key):
        k = tuple(id(o) for o in key[1:]) + (key[0],)
        if k not in self.index:
            self.index[k] = len(self.units)
            self.units.append(key)
        return self.index[k]

    def unit_bc(self, *mods):
        return self._unit(("bc",) + mods)

    def unit_plain(self, conv):
        return self._unit(("plain", conv))

    def unit_linear(self, lin, bn):
        return self._unit(("linear", lin, bn))

    def unit_shape(self, i):
        """(K, C as stored, kh, kw)"""
        key = self.units[i]
        if key[0] == "linear":
            return key[1].out_features, key[1].in_features, 1, 1
        convs = [m.conv for m in key[1:]] if key[0] == "bc" else [key[1]]
        K = sum(c.out_channels for c in convs)
        c0 = convs[0]
        return K, (c0.in_channels + 3) // 4 * 4, c0.kernel_size[0], c0.kernel_size[1]

    def _fold_unit(self, key):
        if key[0] == "plain":
            return pack_weight(key[1].weight.detach()), key[1].bias.detach().clone()
        if key[0] == "linear":
            lin, bn = key[1], key[2]
            w, b = fold_conv_bn(lin.weight.detach(), bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, bn.eps)
            return w.reshape(w.shape[0], 1, 1, w.shape[1]).contiguous(), b
        ws, bs = [], []
        for m in key[1:]:
            w, b = fold_conv_bn(m.conv.weight.detach(), m.bn.weight.detach(), m.bn.bias.detach(), m.bn.running_mean, m.bn.running_var,
                                m.bn.eps)
            ws.append(pack_weight(w))
            bs.append(b)
        return torch.cat(ws, 0).contiguous(), torch.cat(bs, 0).contiguous()

    def _sources(self):
        return [t for t in list(self.model.parameters()) + list(self.model.buffers()) if t.is_floating_point()]

    def weights(self):
        """The folded (weight, bias) of every unit, refolded when a source tensor changed since the last fold."""
        s = plans.stamp(self._sources())
        if self.folded is None or s != self.stamp:
            with torch.no_grad():
                new = [self._fold_unit(k) for k in self.units]
                if self.folded is None or any(o[0].shape != n[0].shape or o[0].device != n[0].device for o, n in zip(self.folded, new)):
                    self.folded, self.programs = new, {}
                else:
                    for (ow, ob), (nw, nb) in zip(self.folded, new):      # same storage: the launch lists keep their pointers
                        ow.copy_(nw)
                        ob.copy_(nb)
            self.stamp = s
        return self.folded

    # ---- launch lists
    def _arena(self, dev, H, W, need):
        a = self.arenas.get((H, W))
        if a is None or any(a[k].numel() < v or a[k].device != dev for k, v in need.items()):
            a = {k: L._new(dev, max(v, a[k].numel() if a else 0)) for k, v in need.items()}
            self.arenas[(H, W)] = a
            for key in [k for k in self.programs if k[1:] == (H, W)]:
                del self.programs[key]
        return a

    def program(self, dev, N, H, W):
        prog = self.programs.get((N, H, W))
        if prog is not None:
            return prog
        b = _Builder(self, N, H, W)
        last = _program(b, self.model)
        folded = self.weights()
        arena = self._arena(dev, H, W, b.need)
        lib = L.get()

        def at(buf, off):
            return arena[buf].data_ptr() + 4 * off

        calls = []
        for op in b.ops:
            if op[0] == "conv":
                _, d, unit, x, (buf, off), res = op
                w, bias = folded[unit]
                calls.append((lib.mt_conv2d_fwd, (C.byref(d), at(x.buf, x.off), w.data_ptr(), bias.data_ptr(),
                                                  at(res.buf, res.off) if res is not None else None, at(buf, off))))
            elif op[0] == "maxpool":
                _, x, (buf, off, ld) = op
                calls.append((lib.mt_maxpool2d_fwd, (at(x.buf, x.off), x.ld, at(buf, off), ld, N, x.h, x.w, x.C, 3, 2, 0)))
            else:
                _, x, (buf, off, ld) = op
                calls.append((lib.mt_avgpool_rows, (at(x.buf, x.off), x.ld, at(buf, off), ld, N, x.h * x.w, x.C)))
        prog = {"calls": calls, "in4": arena["in4"].data_ptr(), "lin": at(last.buf, last.off), "keep": (b.ops, arena, folded)}
        self.programs[(N, H, W)] = prog
        return prog

    def out_rows(self, dev, T):
        o = self.outs.get(T)
        if o is None or o.device != dev:
            o = self.outs[T] = L._new(dev, T, 512)
        return o

    @torch.no_grad()
    def run(self, src, is_u8, strides, T, H, W, standardize):
        """src: device tensor holding [T][H][W][3] elements at element strides (t, h, w, c) -> [T, 512] fp32 (this engine's buffer,
        overwritten by the next call with the same T)."""
        check_side(H, W)
        dev = src.device
        st = L.stream_ptr()
        self.weights()
        out = self.out_rows(dev, T)
        es = src.element_size()
        for t0 in range(0, T, self.chunk):
            n = min(self.chunk, T - t0)
            prog = self.program(dev, n, H, W)
            L.mt.face_ingest(src.data_ptr() + t0 * strides[0] * es, int(is_u8), strides[0], strides[1], strides[2], strides[3], n, H, W,
                             int(standardize), prog["in4"], st)
            for fn, args in prog["calls"]:
                rc = fn(*args, st)
                if rc:
                    L.check(rc, fn.__name__)
            L.mt.l2_normalize_rows(prog["lin"], 512, out[t0:], 512, n, 512, NORM_EPS, st)
        return out
