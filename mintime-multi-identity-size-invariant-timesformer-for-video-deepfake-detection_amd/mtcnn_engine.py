"""The launch sequence of the MTCNN detector (mtcnn.py) on csrc/mtcnn.hip and mt_conv2d_fwd.  Inference only.

  * One fused launch per pyramid level (mt_mtcnn_pnet) appends the candidates of every frame to per-(image, level) lists; neither
    a resized level nor a map is written.  NMS at 0.5 per (image, level) pours the survivors into one list per image, NMS at 0.7
    per image follows, then refine + rerec + pad.
  * R-Net and O-Net are mt_conv2d_fwd launches over the full capacity (rows past a list's count hold zeros or stale values and are
    never read back), the dense layers as convolutions over the 3 x 3 grid: the package flattens in (w, h, c) order, so the dense
    weights are permuted once to the channels-last (h, w, c) row.  The two heads are stacked along K and padded to 8.  PReLU and
    the ceil-mode pools are mt_mtcnn_prelu_pool, which does skip the unused rows.
  * Every list is a segment per image, so a frame's boxes never depend on its neighbours in the batch; mt_mtcnn_finalize packs the
    per-image results into one `Detections`.
  * Weights are repacked under `plans.stamp(...)` of the module's tensors, into the same storage.  After the first call at a
    (N, H, W) nothing is allocated and nothing is read back; `Detections.raise_on_error()` is the only synchronising call.
"""
import ctypes as C

import torch

from . import lib as L
from . import plans
from .facenet_engine import pack_weight

REC = 12                                   # floats per record: x1 y1 x2 y2 score reg[4] key 0 0 (include/mintime_hip.h)
PNET_FLOATS = 6632
MAX_LIST = 1024                            # mt_mtcnn_nms: boxes per segment
ERR_BITS = {1: "stage 1: candidates of one (image, level) exceed max_candidates",
            2: "stage 1: candidates of one image after the per-level NMS exceed max_candidates",
            4: "stage 2: boxes of one image kept by R-Net exceed max_refined",
            8: "stage 3: boxes of one image exceed max_refined",
            16: "the batch's faces exceed max_faces"}

# (kind, name, kernel) / (kind, name, pool k, pool s); "head" = the two dense heads stacked
RNET = [("conv", "conv1", 3), ("pp", "prelu1", 3, 2), ("conv", "conv2", 3), ("pp", "prelu2", 3, 2), ("conv", "conv3", 2),
        ("pp", "prelu3", 1, 1), ("conv", "dense4", 3), ("pp", "prelu4", 1, 1), ("conv", "head", 1)]
ONET = [("conv", "conv1", 3), ("pp", "prelu1", 3, 2), ("conv", "conv2", 3), ("pp", "prelu2", 3, 2), ("conv", "conv3", 3),
        ("pp", "prelu3", 2, 2), ("conv", "conv4", 2), ("pp", "prelu4", 1, 1), ("conv", "dense5", 3), ("pp", "prelu5", 1, 1),
        ("conv", "head", 1)]


def pyramid_scales(H, W, min_face_size=20, factor=0.709):
    """The package's scale pyramid, in Python floats."""
    m = 12.0 / min_face_size
    minl = min(H, W) * m
    s, out = m, []
    while minl >= 12:
        out.append(s)
        s = s * factor
        minl = minl * factor
    return out


def level_size(H, W, s):
    return int(H * s + 1), int(W * s + 1)


def map_size(side):
    """P-Net map side of a level side: conv1, ceil-mode pool, conv2, conv3."""
    return (side - 1) // 2 - 4


def pool_size(n, k, s):
    """MaxPool(k, s, ceil_mode=True) output side."""
    if k == 1:
        return n
    o = -(-(n - k) // s) + 1
    return o - 1 if (o - 1) * s >= n else o


def pack_pnet(p):
    """P-Net as the 6632 floats of mt_mtcnn_pnet: every filter as [ky][kx][ci][co]."""
    def f(w):
        return w.detach().permute(2, 3, 1, 0).reshape(-1)
    w4 = torch.cat([p.conv4_1.weight.detach().reshape(2, 32), p.conv4_2.weight.detach().reshape(4, 32)], 0).t().reshape(-1)
    b4 = torch.cat([p.conv4_1.bias.detach(), p.conv4_2.bias.detach()])
    out = torch.cat([f(p.conv1.weight), p.conv1.bias.detach(), p.prelu1.weight.detach(), f(p.conv2.weight), p.conv2.bias.detach(),
                     p.prelu2.weight.detach(), f(p.conv3.weight), p.conv3.bias.detach(), p.prelu3.weight.detach(), w4, b4]).contiguous().float()
    assert out.numel() == PNET_FLOATS
    return out


def pack_dense(lin, c):
    """A dense layer over the package's (w, h, c) flatten of a 3 x 3 x c grid, as a [K][3][3][c] convolution over channels-last rows."""
    K = lin.weight.shape[0]
    return lin.weight.detach().reshape(K, 3, 3, c).permute(0, 2, 1, 3).contiguous(), lin.bias.detach().clone()


def pack_head(cls, reg):
    """dense*_1 (2 logits) and dense*_2 (4 regression values) stacked along K, padded to 8."""
    w = torch.cat([cls.weight.detach(), reg.weight.detach()], 0)
    b = torch.cat([cls.bias.detach(), reg.bias.detach()])
    w = torch.nn.functional.pad(w, (0, 0, 0, 2))
    return w.reshape(8, 1, 1, w.shape[1]).contiguous(), torch.nn.functional.pad(b, (0, 2)).contiguous()


def pack_net(net, spec):
    """{layer name: (weight, bias) or slope} of R-Net / O-Net in the layouts the launches take."""
    out = {}
    for op in spec:
        name = op[1]
        if op[0] == "pp":
            out[name] = getattr(net, name).weight.detach().clone().contiguous()
        elif name == "head":
            heads = ("dense5_1", "dense5_2") if hasattr(net, "dense5_1") else ("dense6_1", "dense6_2")
            out[name] = pack_head(getattr(net, heads[0]), getattr(net, heads[1]))
        elif name.startswith("dense"):
            m = getattr(net, name)
            out[name] = pack_dense(m, m.weight.shape[1] // 9)
        else:
            m = getattr(net, name)
            out[name] = (pack_weight(m.weight.detach()), m.bias.detach().clone())
    return out


class Detections:
    """What `detect_device` returns: device tensors of the module, overwritten by its next call at the same batch shape.
    boxes [max_faces, 4] fp32 (x1, y1, x2, y2), probs [max_faces], frame_index [max_faces] int32 (-1 on unused rows), count (device
    int32 scalar), image_counts [N] int32; rows are image-major, within an image in the order of the stage-3 NMS."""

    def __init__(self, boxes, probs, frame_index, count, image_counts, err):
        self.boxes, self.probs, self.frame_index, self.count, self.image_counts = boxes, probs, frame_index, count, image_counts
        self._err = err

    def error_word(self) -> int:
        """The sticky overflow bits (mtcnn_engine.ERR_BITS) set since they were last read; synchronises and clears them."""
        e = int(self._err.cpu()[0])
        if e:
            L.zero_(self._err)
        return e

    def raise_on_error(self):
        e = self.error_word()
        if e:
            raise L.MintimeHipError("MTCNN: capacity overflow, results are incomplete -- " +
                                    "; ".join(msg for bit, msg in ERR_BITS.items() if e & bit))


class Engine:
    def __init__(self, model):
        self.model = model
        self.packed, self.stamp = None, None
        self.states = {}
        self.err = None
        self.debug = None                 # a dict: receives clones of the lists after every stage (tests; allocates)

    # ---- weights
    def _sources(self):
        return [t for t in self.model.parameters()]

    def weights(self):
        s = plans.stamp(self._sources())
        if self.packed is None or s != self.stamp:
            m = self.model
            with torch.no_grad():
                new = {"pnet": pack_pnet(m.pnet), "rnet": pack_net(m.rnet, RNET), "onet": pack_net(m.onet, ONET)}
            flat_new, flat_old = _flatten(new), _flatten(self.packed) if self.packed is not None else None
            if flat_old is None or any(o.shape != n.shape or o.device != n.device for o, n in zip(flat_old, flat_new)):
                self.packed, self.states = new, {}
            else:
                for o, n in zip(flat_old, flat_new):          # same storage: the launch lists keep their pointers
                    o.copy_(n)
            self.stamp = s
        return self.packed

    # ---- launch lists
    def _net(self, dev, name, spec, rows, side, x_in, counts, cap):
        """The launches of R-Net / O-Net over `rows` crops of side x side x 4 in x_in -> (calls, head [rows, 8])."""
        packed = self.packed[name]
        lib = L.get()
        h = w = side
        c = 4
        shapes = []
        for op in spec:
            if op[0] == "conv":
                k = op[2]
                h, w, c = h - k + 1, w - k + 1, packed[op[1]][0].shape[0]
            else:
                h, w = pool_size(h, op[2], op[3]), pool_size(w, op[2], op[3])
            shapes.append((h, w, c))
        bufs = [L._new(dev, rows * max(hh * ww * cc for hh, ww, cc in shapes[i::2])) for i in (0, 1)]
        calls, keep = [], [bufs]
        src, (h, w, c) = x_in, (side, side, 4)
        for i, op in enumerate(spec):
            ho, wo, co = shapes[i]
            dst = bufs[i % 2]
            if op[0] == "conv":
                wt, bias = packed[op[1]]
                d = L.Conv2dDesc()
                d.N, d.H, d.W, d.C, d.Ho, d.Wo, d.K = rows, h, w, c, ho, wo, co
                d.kh = d.kw = op[2]
                d.sh = d.sw = 1
                d.ph = d.pw = 0
                d.act, d.res_scale = 0, 1.0
                d.ldx, d.ldy, d.ldr = c, co, 0
                keep.append(d)
                calls.append((lib.mt_conv2d_fwd, (C.byref(d), src.data_ptr(), wt.data_ptr(), bias.data_ptr(), None, dst.data_ptr())))
            else:
                calls.append((lib.mt_mtcnn_prelu_pool, (src.data_ptr(), dst.data_ptr(), packed[op[1]].data_ptr(), rows, h, w, c, op[2], op[3],
                                                        counts.data_ptr(), cap)))
            src, (h, w, c) = dst, (ho, wo, co)
        assert (h, w, c) == (1, 1, 8), (name, h, w, c)
        return calls, src, keep

    def state(self, dev, N, H, W):
        key = (str(dev), N, H, W)
        st = self.states.get(key)
        if st is not None:
            return st
        m = self.model
        self.weights()
        scales = pyramid_scales(H, W, m.min_face_size, m.factor)
        if not scales:
            raise ValueError(f"MTCNN: {H} x {W} frames hold no pyramid level at min_face_size = {m.min_face_size}")
        Lv, cap, cap3 = len(scales), m.max_candidates, m.max_refined
        if self.err is None or self.err.device != dev:
            self.err = L.zeros(1, torch.int32, dev)
        st = {"levels": [(level_size(H, W, s) + (float(s),)) for s in scales], "cap": cap, "cap3": cap3}
        st["u8"] = torch.empty(N, H, W, 3, dtype=torch.uint8, device=dev)
        cnt = L.zeros(N * Lv + 4 * N, torch.int32, dev)
        st["cnt"] = cnt
        st["cnt1"], st["cntA"], st["cntB"], st["cntC"], st["cntD"] = (cnt[:N * Lv], cnt[N * Lv:N * Lv + N], cnt[N * Lv + N:N * Lv + 2 * N],
                                                                     cnt[N * Lv + 2 * N:N * Lv + 3 * N], cnt[N * Lv + 3 * N:])
        st["rec1"] = L.zeros((N * Lv, cap, REC), torch.float32, dev)
        st["recA"] = L.zeros((N, cap, REC), torch.float32, dev)
        st["recB"] = L.zeros((N, cap, REC), torch.float32, dev)
        st["recC"] = L.zeros((N, cap3, REC), torch.float32, dev)
        st["recD"] = L.zeros((N, cap3, REC), torch.float32, dev)
        st["winB"] = L.zeros((N, cap, 4), torch.int32, dev)
        st["winC"] = L.zeros((N, cap3, 4), torch.int32, dev)
        st["x24"] = L._new(dev, N * cap, 24, 24, 4)
        st["x48"] = L._new(dev, N * cap3, 48, 48, 4)
        st["rnet"] = self._net(dev, "rnet", RNET, N * cap, 24, st["x24"], st["cntB"], cap)
        st["onet"] = self._net(dev, "onet", ONET, N * cap3, 48, st["x48"], st["cntC"], cap3)
        mf = m.max_faces
        st["out"] = Detections(L._new(dev, mf, 4), L._new(dev, mf), torch.empty(mf, dtype=torch.int32, device=dev),
                               torch.empty((), dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev), self.err)
        self.states[key] = st
        return st

    def _snap(self, name, rec, cnt):
        if self.debug is not None:
            self.debug[name] = (rec.clone(), cnt.clone())

    @torch.no_grad()
    def run(self, frames):
        """frames [N, H, W, 3] uint8 (or fp32 holding integer values), contiguous, on the device -> Detections."""
        dev = frames.device
        N, H, W, _ = frames.shape
        self.weights()
        st = self.state(dev, N, H, W)
        if frames.dtype != torch.uint8 or not frames.is_contiguous():
            st["u8"].copy_(frames)
            frames = st["u8"]
        mt, stream = L.mt, L.stream_ptr()
        t0, t1, t2 = (float(t) for t in self.model.thresholds)
        cap, cap3, levels = st["cap"], st["cap3"], st["levels"]
        Lv = len(levels)
        pn = self.packed["pnet"]
        L.zero_(st["cnt"][:N * Lv + N])
        for l, (hs, ws, s) in enumerate(levels):
            mt.mtcnn_pnet(frames, N, H, W, hs, ws, s, l, Lv, pn, t0, st["rec1"], st["cnt1"], cap, self.err, None, None, stream)
        self._snap("cand", st["rec1"], st["cnt1"])
        mt.mtcnn_nms(st["rec1"], st["cnt1"], N * Lv, cap, Lv, 0, 0.5, st["recA"], st["cntA"], cap, None, self.err, 2, stream)
        mt.mtcnn_nms(st["recA"], st["cntA"], N, cap, 1, 0, 0.7, st["recB"], st["cntB"], cap, None, self.err, 2, stream)
        mt.mtcnn_boxes(st["recB"], st["cntB"], N, cap, 1, H, W, st["winB"], stream)
        self._snap("stage1", st["recB"], st["cntB"])
        mt.mtcnn_crop(frames, N, H, W, st["winB"], st["cntB"], cap, 24, st["x24"], stream)
        head = self._run_net(st["rnet"], stream)
        mt.mtcnn_score(head, 8, st["recB"], st["winB"], st["cntB"], N, cap, H, W, t1, stream)
        mt.mtcnn_nms(st["recB"], st["cntB"], N, cap, 1, 0, 0.7, st["recC"], st["cntC"], cap3, None, self.err, 4, stream)
        mt.mtcnn_boxes(st["recC"], st["cntC"], N, cap3, 2, H, W, st["winC"], stream)
        self._snap("stage2", st["recC"], st["cntC"])
        mt.mtcnn_crop(frames, N, H, W, st["winC"], st["cntC"], cap3, 48, st["x48"], stream)
        head = self._run_net(st["onet"], stream)
        mt.mtcnn_score(head, 8, st["recC"], st["winC"], st["cntC"], N, cap3, H, W, t2, stream)
        mt.mtcnn_boxes(st["recC"], st["cntC"], N, cap3, 3, H, W, None, stream)
        mt.mtcnn_nms(st["recC"], st["cntC"], N, cap3, 1, 1, 0.7, st["recD"], st["cntD"], cap3, None, self.err, 8, stream)
        self._snap("stage3", st["recD"], st["cntD"])
        o = st["out"]
        mt.mtcnn_finalize(st["recD"], st["cntD"], N, cap3, self.model.max_faces, o.boxes, o.probs, o.frame_index, o.count, o.image_counts,
                          self.err, 16, stream)
        return o

    @staticmethod
    def _run_net(net, stream):
        calls, head, _ = net
        for fn, args in calls:
            rc = fn(*args, stream)
            if rc:
                L.check(rc, fn.__name__)
        return head


def _flatten(packed):
    out = [packed["pnet"]]
    for name in ("rnet", "onet"):
        for v in packed[name].values():
            out.extend(v if isinstance(v, tuple) else (v,))
    return out
