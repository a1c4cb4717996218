"""Per-kernel tests of csrc/mtcnn.hip on the device, against tests/mtcnn_ref.py.

Bounds.  u = 2^-24.  A layer whose outputs are bias + a chain of n fused multiply-adds is within (n + 1) u (sum |x w| + |b|) of its
exact value to first order, plus sum |w| e_in for the error e_in its inputs carry; PReLU adds u |y| and scales e_in by max(1, |a|);
a max-pool passes the largest error of its window; softmax over two logits moves by at most (e_0 + e_1) / 4 + 8 u.  The bound is
propagated position by position through the fp64 restatement (`Bounded`) and asserted with no slack factor beyond 2 u absolute.
The resized level is an exact integer sum, one division, one subtraction and an exact scaling: 3 u (it is below 1 in magnitude).
mt_conv2d_fwd states (kh kw C + 4) u for its own chain; R-Net and O-Net use that n.
Decisions (candidate sets, NMS picks and order, box arithmetic, pad windows) are compared exactly, on the device's own inputs."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mintime_amd
from mintime_amd import lib as L
from mintime_amd import mtcnn_engine as E
from tests import mtcnn_ref as R

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
SEED = 20
REC = E.REC


@pytest.fixture(scope="module")
def sd32():
    return {k: v.float() for k, v in R.healthy_weights(SEED).items()}


@pytest.fixture(scope="module")
def sd64(sd32):
    return {k: v.double() for k, v in sd32.items()}              # the fp32 weights, exactly


@pytest.fixture(scope="module")
def det(sd32):
    d = mintime_amd.MTCNN(device="cuda", thresholds=[0.6, 0.7, 0.7], max_candidates=128, max_refined=32, max_faces=32)
    d.load_state_dict(sd32)
    return d


class Bounded:
    """A value (fp64, exact up to fp64) and a first-order bound of the fp32 implementation's error, layer by layer."""

    def __init__(self, v, e):
        self.v, self.e = v, e

    def conv(self, w, b, n):
        v = F.conv2d(self.v, w, b)
        mag = F.conv2d(self.v.abs(), w.abs(), b.abs())
        return Bounded(v, (n + 1) * U * mag + F.conv2d(self.e, w.abs()))

    def linear(self, w, b, n):
        v = F.linear(self.v, w, b)
        return Bounded(v, (n + 1) * U * F.linear(self.v.abs(), w.abs(), b.abs()) + F.linear(self.e, w.abs()))

    def prelu(self, a):
        v = F.prelu(self.v, a)
        shape = [1, -1] + [1] * (self.v.dim() - 2)
        return Bounded(v, self.e * a.abs().clamp(min=1).reshape(shape) + U * v.abs())

    def pool(self, k, s):
        return Bounded(F.max_pool2d(self.v, k, s, ceil_mode=True), F.max_pool2d(self.e, k, s, ceil_mode=True))

    def flatten(self):
        return Bounded(R.flatten_whc(self.v), R.flatten_whc(self.e))


def _prob(logits):
    """softmax channel 1 and its bound from two bounded logits [.., 2, ..] on dim 1"""
    p = torch.softmax(logits.v, dim=1)[:, 1]
    return p, 0.25 * (logits.e[:, 0] + logits.e[:, 1]) + 8 * U


def pnet_bounded(sd, level):
    p = R._sd(sd, "pnet", torch.float64)
    x = Bounded(level, torch.full_like(level, 3 * U))
    x = x.conv(p["conv1.weight"], p["conv1.bias"], 27).prelu(p["prelu1.weight"]).pool(2, 2)
    x = x.conv(p["conv2.weight"], p["conv2.bias"], 90).prelu(p["prelu2.weight"])
    x = x.conv(p["conv3.weight"], p["conv3.bias"], 144).prelu(p["prelu3.weight"])
    return _prob(x.conv(p["conv4_1.weight"], p["conv4_1.bias"], 32)), x.conv(p["conv4_2.weight"], p["conv4_2.bias"], 32)


def rnet_bounded(sd, crops):
    p = R._sd(sd, "rnet", torch.float64)
    x = Bounded(crops, torch.full_like(crops, 3 * U))
    x = x.conv(p["conv1.weight"], p["conv1.bias"], 39).prelu(p["prelu1.weight"]).pool(3, 2)
    x = x.conv(p["conv2.weight"], p["conv2.bias"], 255).prelu(p["prelu2.weight"]).pool(3, 2)
    x = x.conv(p["conv3.weight"], p["conv3.bias"], 195).prelu(p["prelu3.weight"]).flatten()
    x = x.linear(p["dense4.weight"], p["dense4.bias"], 579).prelu(p["prelu4.weight"])
    return _prob(x.linear(p["dense5_1.weight"], p["dense5_1.bias"], 131)), x.linear(p["dense5_2.weight"], p["dense5_2.bias"], 131)


def onet_bounded(sd, crops):
    p = R._sd(sd, "onet", torch.float64)
    x = Bounded(crops, torch.full_like(crops, 3 * U))
    x = x.conv(p["conv1.weight"], p["conv1.bias"], 39).prelu(p["prelu1.weight"]).pool(3, 2)
    x = x.conv(p["conv2.weight"], p["conv2.bias"], 291).prelu(p["prelu2.weight"]).pool(3, 2)
    x = x.conv(p["conv3.weight"], p["conv3.bias"], 579).prelu(p["prelu3.weight"]).pool(2, 2)
    x = x.conv(p["conv4.weight"], p["conv4.bias"], 259).prelu(p["prelu4.weight"]).flatten()
    x = x.linear(p["dense5.weight"], p["dense5.bias"], 1155).prelu(p["prelu5.weight"])
    return _prob(x.linear(p["dense6_1.weight"], p["dense6_1.bias"], 259)), x.linear(p["dense6_2.weight"], p["dense6_2.bias"], 259)


def _within(got, ref, bound, what):
    d = (got.double().cpu() - ref).abs()
    lim = bound + 2 * U
    worst = float((d / lim).max())
    print(f"{what}: max error {float(d.max()):.2e}, largest error / bound {worst:.2e}")
    assert worst <= 1.0, what


def _run_pnet(det, frames, hs, ws, scale=0.6, thr=2.0, cap=64, level=0, levels=1, debug=True):
    """One mt_mtcnn_pnet launch -> (rec, counts, err, level, maps)."""
    dev = frames.device
    N, H, W, _ = frames.shape
    hm, wm = E.map_size(hs), E.map_size(ws)
    rec = torch.zeros(N * levels, cap, REC, device=dev)
    cnt = torch.zeros(N * levels, dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    lvl = torch.full((N, hs, ws, 3), 9.0, device=dev) if debug else None
    maps = torch.full((N, 5, hm, wm), 9.0, device=dev) if debug else None
    L.mt.mtcnn_pnet(frames, N, H, W, hs, ws, scale, level, levels, det.engine().weights()["pnet"], thr, rec, cnt, cap, err, lvl, maps)
    return rec, cnt, err, lvl, maps


# 12 x 12: one output; 13 x 17: odd conv1 output, so a partial ceil-mode pool window; 58 x 77; 90 x 110: map 40 x 50 = 3 x 4 tiles,
# the last of each axis ragged
@pytest.mark.parametrize("size,frame", [((12, 12), (96, 128)), ((13, 17), (96, 128)), ((58, 77), (96, 128)), ((90, 110), (150, 181))])
def test_pnet_maps_and_level_against_fp64(det, sd64, size, frame):
    hs, ws = size
    frames = R.make_frames(SEED, 2, *frame)
    assert not torch.equal(frames[0], frames[1])
    _, _, _, lvl, maps = _run_pnet(det, frames.cuda(), hs, ws)
    ref_level = R.normalise(R.area_resize(frames.permute(0, 3, 1, 2).double(), hs, ws))
    _within(lvl.permute(0, 3, 1, 2), ref_level, torch.full_like(ref_level, 3 * U), f"level {hs} x {ws}")
    (prob, eprob), reg = pnet_bounded(sd64, ref_level)
    assert maps.shape[2:] == prob.shape[1:] == (E.map_size(hs), E.map_size(ws))
    _within(maps[:, 0], prob, eprob, f"prob map of level {hs} x {ws}")
    _within(maps[:, 1:], reg.v, reg.e, f"reg map of level {hs} x {ws}")
    assert float(prob.max() - prob.min()) > 0.2 or prob.numel() < 100          # the maps are not flat: the test weights are healthy


@pytest.fixture(scope="module")
def emitted(det):
    """The candidates of one multi-tile level of two frames, at the 0.8 quantile of the device's own probabilities."""
    frames = R.make_frames(SEED, 2, 150, 181).cuda()
    hs, ws, scale = 90, 110, 0.6
    _, _, _, _, maps = _run_pnet(det, frames, hs, ws, scale)
    thr = float(np.float32(torch.quantile(maps[:, 0].reshape(-1), 0.8).item()))
    rec, cnt, err, _, maps2 = _run_pnet(det, frames, hs, ws, scale, thr=thr, cap=1024, level=2, levels=3)
    assert torch.equal(maps, maps2)                                           # the same bits whatever the threshold
    return {"rec": rec, "cnt": cnt, "err": err, "maps": maps.cpu(), "thr": thr, "scale": scale, "levels": 3, "level": 2}


def test_candidate_emission_is_the_fp32_logic_on_the_devices_maps(emitted):
    maps, thr = emitted["maps"], emitted["thr"]
    prob = maps[:, 0]
    wm = prob.shape[2]
    cnt = emitted["cnt"].cpu().reshape(2, 3)
    assert int(emitted["err"].item()) == 0 and cnt[:, :2].eq(0).all()
    for n in range(2):
        idx = torch.nonzero(prob[n] >= torch.tensor(thr))
        want = {}
        boxes = R.candidate_boxes(idx[:, 1], idx[:, 0], emitted["scale"])
        for (y, x), b in zip(idx.tolist(), boxes):
            want[(2 << 24) | (y * wm + x)] = (b, prob[n, y, x], maps[n, 1:, y, x])
        assert int(cnt[n, 2]) == len(want) > 100
        rows = emitted["rec"][n * 3 + 2, :len(want)].cpu()
        keys = rows[:, 9].contiguous().view(torch.int32).tolist()
        assert sorted(keys) == sorted(want)                                   # as a set: the append order is not defined
        for r, k in zip(rows, keys):
            b, p, g = want[k]
            assert torch.equal(r[:4], b) and r[4] == p and torch.equal(r[5:9], g) and not r[10:].any()


def _segments(dev):
    """Five hand-made segments of capacity 64: tied scores, empty, one box, exactly at capacity, a count above the capacity with
    dropped rows (score -1) inside."""
    g = torch.Generator().manual_seed(5)
    cap = 64
    rec = torch.zeros(5, cap, REC)
    xy = 60 * torch.rand(5, cap, 2, generator=g)
    wh = 8 + 30 * torch.rand(5, cap, 2, generator=g)
    rec[:, :, 0:2], rec[:, :, 2:4] = xy, xy + wh
    rec[:, :, 4] = torch.rand(5, cap, generator=g)
    rec[0, :40:4, 4] = 1.0                                                    # ten ties at a saturated score
    rec[0, 1:40:4, 4] = rec[0, 2, 4]
    rec[4, 5:30:3, 4] = -1.0
    keys = torch.stack([torch.randperm(cap, generator=g) for _ in range(5)]).to(torch.int32)
    rec[:, :, 9] = keys.view(torch.float32)
    cnt = torch.tensor([40, 0, 1, 64, 70], dtype=torch.int32)
    return rec.to(dev), cnt.to(dev), cap


def _ref_picks(rec, n, thr, form):
    rows = rec[:n]
    alive = torch.nonzero(rows[:, 4] >= 0).reshape(-1)
    r = rows[alive]
    keep = R.nms(r[:, :4], r[:, 4], r[:, 9].contiguous().view(torch.int32), thr, form)
    return alive[keep].tolist()


@pytest.mark.parametrize("form", [0, 1])
def test_nms_picks_and_order_are_exact(emitted, form):
    dev = emitted["rec"].device
    for rec, cnt, cap, thr in [(*_segments(dev), 0.5), (*_segments(dev), 0.7), (emitted["rec"], emitted["cnt"], 1024, 0.5),
                               (emitted["rec"], emitted["cnt"], 1024, 0.7)]:
        segs = rec.shape[0]
        out = torch.full((segs, cap, REC), 7.0, device=dev)
        kept = torch.full((segs,), -5, dtype=torch.int32, device=dev)
        picks = torch.full((segs, cap), -7, dtype=torch.int32, device=dev)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        L.mt.mtcnn_nms(rec, cnt, segs, cap, 1, form, thr, out, kept, cap, picks, err, 4)
        rec_h, out_h, picks_h = rec.cpu(), out.cpu(), picks.cpu()
        assert int(err.item()) == 0
        for s in range(segs):
            n = min(int(cnt[s]), cap)
            want = _ref_picks(rec_h[s], n, thr, form)
            assert int(kept[s]) == len(want) and picks_h[s, :len(want)].tolist() == want and picks_h[s, len(want):].eq(-1).all()
            assert torch.equal(out_h[s, :len(want)].view(torch.int32), rec_h[s][want].view(torch.int32))
            assert out_h[s, len(want):].eq(7.0).all()
        assert 0 < int(kept.max()) and int(kept.sum()) < int(cnt.clamp(max=cap).sum())      # something was suppressed


def test_nms_groups_pour_into_one_list_and_overflow_is_flagged():
    rec, cnt, cap = _segments(torch.device("cuda"))
    rec, cnt = rec[:4].clone(), cnt[:4].clone()
    keys = rec[:, :, 9].cpu().contiguous().view(torch.int32) + 1000 * torch.arange(4, dtype=torch.int32)[:, None]      # unique in a group
    rec[:, :, 9] = keys.view(torch.float32).cuda()
    rec_h = rec.cpu()
    ref = [[int(keys[s, i]) for i in _ref_picks(rec_h[s], int(cnt[s]), 0.5, 0)] for s in range(4)]
    want = [len(ref[0]) + len(ref[1]), len(ref[2]) + len(ref[3])]
    assert max(want) > 16
    for cap_out in (128, 16):
        guard = torch.full((2 * cap_out + 32, REC), 3.0, device="cuda")
        out = guard[16:16 + 2 * cap_out].view(2, cap_out, REC)
        kept = torch.zeros(2, dtype=torch.int32, device="cuda")
        err = torch.zeros(1, dtype=torch.int32, device="cuda")
        L.mt.mtcnn_nms(rec, cnt, 4, cap, 2, 0, 0.5, out, kept, cap_out, None, err, 2)
        assert kept.tolist() == want
        assert guard[:16].eq(3.0).all() and guard[16 + 2 * cap_out:].eq(3.0).all()
        for gi in range(2):
            n = min(want[gi], cap_out)
            got = out[gi, :n, 9].contiguous().view(torch.int32).tolist()
            assert set(got) <= set(ref[2 * gi] + ref[2 * gi + 1]) and len(set(got)) == n
            assert out[gi, n:].eq(3.0).all()
        assert int(err.item()) == (2 if max(want) > cap_out else 0)


def _random_records(segs, cap, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    rec = torch.zeros(segs, cap, REC)
    xy = torch.rand(segs, cap, 2, generator=g) * torch.tensor([W, H]) - 10
    wh = 3 + 50 * torch.rand(segs, cap, 2, generator=g)
    rec[:, :, 0:2], rec[:, :, 2:4] = xy, xy + wh
    rec[:, :, 4] = torch.rand(segs, cap, generator=g)
    rec[:, :, 5:9] = 0.3 * torch.randn(segs, cap, 4, generator=g)
    return rec


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_box_arithmetic_is_bit_equal_to_torch_fp32(mode):
    H, W, segs, cap = 96, 128, 3, 50
    rec = _random_records(segs, cap, H, W, 11 + mode)
    rec[0, :20, :4] = rec[0, :20, :4].round()                                 # stage-1 boxes are whole numbers
    cnt = torch.tensor([50, 0, 33], dtype=torch.int32)
    d_rec, win = rec.cuda(), torch.full((segs, cap, 4), -3, dtype=torch.int32, device="cuda")
    L.mt.mtcnn_boxes(d_rec, cnt.cuda(), segs, cap, mode, H, W, win)
    got, win = d_rec.cpu(), win.cpu()
    for s in range(segs):
        n = int(cnt[s])
        b = R.refine(rec[s, :n, :4], rec[s, :n, 5:9], 0 if mode == 1 else 1)
        b = R.rerec(b) if mode != 3 else b
        assert torch.equal(got[s, :n, :4].view(torch.int32), b.view(torch.int32))
        assert torch.equal(got[s, :n, 4:], rec[s, :n, 4:]) and torch.equal(got[s, n:], rec[s, n:])
        assert torch.equal(win[s, :n].long(), R.pad(b, H, W)) and win[s, n:].eq(0).all()


def test_crop_and_resample_against_fp64():
    H, W = 96, 128
    frames = R.make_frames(SEED, 2, H, W)
    boxes = torch.tensor([[30.2, 40.7, 40.9, 53.1],        # smaller than 24: upsampling
                          [20.0, 10.5, 81.3, 71.9],        # larger
                          [-9.5, 30.0, 25.0, 60.0],        # cut by the left edge
                          [50.0, -7.2, 90.0, 20.0],        # the top
                          [100.0, 20.0, 140.6, 70.0],      # the right
                          [40.0, 70.0, 80.0, 120.3],       # the bottom
                          [60.7, 30.0, 59.2, 50.0],        # ex <= x - 1: no pixel (deviation (c))
                          [30.0, 80.9, 50.0, 79.1]])       # ey <= y - 1
    cap = 10
    rec = torch.zeros(2, cap, REC)
    rec[:, :8, :4] = boxes
    cnt = torch.tensor([8, 7], dtype=torch.int32).cuda()
    d_rec, win = rec.cuda(), torch.zeros(2, cap, 4, dtype=torch.int32, device="cuda")
    L.mt.mtcnn_boxes(d_rec, cnt, 2, cap, 0, H, W, win)
    assert torch.equal(d_rec.cpu(), rec)
    x64 = frames.permute(0, 3, 1, 2).double()
    for S in (24, 48):
        guard = torch.full((2 * cap * S * S * 4 + 64,), 5.0, device="cuda")
        out = guard[32:-32].view(2 * cap, S, S, 4)
        L.mt.mtcnn_crop(frames.cuda(), 2, H, W, win, cnt, cap, S, out)
        assert guard[:32].eq(5.0).all() and guard[-32:].eq(5.0).all() and out[..., 3].eq(0).all()
        for n in range(2):
            ref, ok = R.crops(x64, n, win[n, :int(cnt[n])].cpu().long(), S)
            assert ok.tolist() == [True] * 6 + [False] * (int(cnt[n]) - 6)
            got = out[n * cap:(n + 1) * cap, :, :, :3].permute(0, 3, 1, 2)
            _within(got[:int(cnt[n])], ref, torch.full_like(ref, 3 * U), f"crops {S} of frame {n}")
            assert got[6:].eq(0).all()                    # windows without a pixel and rows past the count


@pytest.mark.parametrize("k,s,H,W", [(1, 1, 3, 3), (1, 1, 1, 1), (2, 2, 8, 8), (2, 2, 11, 7), (3, 2, 22, 22), (3, 2, 9, 9), (3, 2, 46, 46),
                                    (3, 2, 21, 21), (3, 2, 10, 13)])
def test_prelu_pool_with_sentinels(k, s, H, W):
    g = torch.Generator().manual_seed(k * 100 + H)
    rows, Cc, cap = 6, 28, 3
    x = torch.randn(rows, H, W, Cc, generator=g)
    a = 0.5 * torch.randn(Cc, generator=g)                                    # negative slopes too: PReLU before the max, not after
    ho, wo = E.pool_size(H, k, s), E.pool_size(W, k, s)
    ref = F.prelu(x.permute(0, 3, 1, 2), a)
    ref = (F.max_pool2d(ref, k, s, ceil_mode=True) if k > 1 else ref).permute(0, 2, 3, 1)
    assert ref.shape == (rows, ho, wo, Cc)
    for counts in (None, torch.tensor([2, 1], dtype=torch.int32).cuda()):
        guard = torch.full((rows * ho * wo * Cc + 64,), 5.0, device="cuda")
        y = guard[32:-32].view(rows, ho, wo, Cc)
        L.mt.mtcnn_prelu_pool(x.cuda(), y, a.cuda(), rows, H, W, Cc, k, s, counts, cap)
        assert guard[:32].eq(5.0).all() and guard[-32:].eq(5.0).all()
        active = [True] * rows if counts is None else [True, True, False, True, False, False]
        for r in range(rows):
            assert torch.equal(y[r].cpu(), ref[r]) if active[r] else y[r].eq(5.0).all()


def test_rnet_and_onet_outputs_against_fp64(det, sd64):
    eng = det.engine()
    N, H, W = 1, 96, 128
    st = eng.state(torch.device("cuda"), N, H, W)
    g = torch.Generator().manual_seed(9)
    for name, side, cnt, fwd in (("rnet", 24, st["cntB"], rnet_bounded), ("onet", 48, st["cntC"], onet_bounded)):
        x_in = st["x24"] if side == 24 else st["x48"]
        rows, n = x_in.shape[0], 12
        crops = R.normalise(F.interpolate(torch.rand(n, 3, 6, 6, generator=g), size=(side, side), mode="bicubic") * 255).clamp(-1, 1).float()
        x_in.zero_()
        x_in[:n, :, :, :3] = crops.permute(0, 2, 3, 1).cuda()
        cnt.fill_(n)
        head = eng._run_net(st[name], L.stream_ptr())[:rows * 8].view(rows, 8)[:n].cpu()
        (prob, eprob), reg = fwd(sd64, crops.double())
        got_prob = torch.softmax(head[:, :2].double(), dim=1)[:, 1]
        _within(got_prob, prob, eprob, f"{name} probabilities")
        _within(head[:, 2:6], reg.v, reg.e, f"{name} regression values")
        assert float(prob.max() - prob.min()) > 0.05
        # the score pass on the device's own head rows: windows without a pixel are dropped
        rec = torch.zeros(N, rows, REC, device="cuda")
        win = torch.tensor([1, 1, 20, 20], dtype=torch.int32, device="cuda").repeat(N, rows, 1).contiguous()
        win[0, 3] = torch.tensor([5, 5, 4, 20], dtype=torch.int32)
        srt = got_prob.sort().values
        thr = float(np.float32(0.5 * (srt[n // 2 - 1] + srt[n // 2]).item()))
        L.mt.mtcnn_score(head.cuda().contiguous(), 8, rec, win, cnt, N, rows, H, W, thr)
        sc = rec[0, :n, 4].cpu()
        keep = got_prob > thr
        keep[3] = False
        assert (sc >= 0).tolist() == keep.tolist() and keep.sum() >= 2
        assert torch.allclose(sc[keep].double(), got_prob[keep], rtol=0, atol=8 * U) and sc[~keep].eq(-1).all()
        assert torch.equal(rec[0, :n, 5:9].cpu(), head[:, 2:6]) and not rec[0, n:].any()
    # the threshold test is strict: equal logits give exactly 0.5 in any arithmetic
    zero_head = torch.zeros(4, 8, device="cuda")
    cnt4 = torch.tensor([4], dtype=torch.int32, device="cuda")
    for thr, alive in ((0.5, False), (0.49999997, True)):
        rec = torch.zeros(1, 4, REC, device="cuda")
        L.mt.mtcnn_score(zero_head, 8, rec, win, cnt4, 1, 4, H, W, thr)
        assert rec[0, :3, 4].eq(0.5 if alive else -1.0).all() and rec[0, 3, 4] == -1.0


def test_argument_errors_return_codes_and_write_nothing(det):
    lib = L.get()
    dev = torch.device("cuda")
    frames = torch.zeros(1, 40, 40, 3, dtype=torch.uint8, device=dev)
    rec = torch.full((4, 8, REC), 2.0, device=dev)
    rec2 = torch.full((4, 8, REC), 2.0, device=dev)
    cnt = torch.full((4,), 3, dtype=torch.int32, device=dev)
    win = torch.full((4, 8, 4), 3, dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    out = torch.full((64 * 24 * 24 * 4,), 2.0, device=dev)
    w = det.engine().weights()["pnet"]
    p = lambda t: t.data_ptr()
    calls = [
        lib.mt_mtcnn_pnet(p(frames), 1, 40, 40, 11, 25, 0.6, 0, 1, p(w), 0.5, p(rec), p(cnt), 8, p(err), None, None, None),       # level < 12
        lib.mt_mtcnn_pnet(p(frames), 1, 40, 40, 25, 25, 0.6, 1, 1, p(w), 0.5, p(rec), p(cnt), 8, p(err), None, None, None),       # level >= levels
        lib.mt_mtcnn_pnet(p(frames), 1, 40, 40, 25, 25, 0.6, 0, 1, None, 0.5, p(rec), p(cnt), 8, p(err), None, None, None),       # null weights
        lib.mt_mtcnn_nms(p(rec), p(cnt), 4, 2048, 1, 0, 0.5, p(rec2), p(cnt), 8, None, p(err), 2, None),                          # cap_in > 1024
        lib.mt_mtcnn_nms(p(rec), p(cnt), 4, 8, 3, 0, 0.5, p(rec2), p(cnt), 8, None, p(err), 2, None),                             # 4 % 3
        lib.mt_mtcnn_nms(p(rec), p(cnt), 4, 8, 1, 2, 0.5, p(rec2), p(cnt), 8, None, p(err), 2, None),                             # form
        lib.mt_mtcnn_nms(p(rec), p(cnt), 4, 8, 1, 0, 0.5, p(rec), p(cnt), 8, None, p(err), 2, None),                              # in place
        lib.mt_mtcnn_boxes(p(rec), p(cnt), 4, 8, 4, 40, 40, p(win), None),                                                        # mode
        lib.mt_mtcnn_boxes(p(rec), p(cnt), 4, 8, 0, 40, 40, None, None),                                                          # pad without win
        lib.mt_mtcnn_crop(p(frames), 1, 40, 40, p(win), p(cnt), 8, 0, p(out), None),                                              # S
        lib.mt_mtcnn_crop(p(frames), 1, 40, 40, p(win), p(cnt), 8, 24, p(out) + 4, None),                                         # alignment
        lib.mt_mtcnn_prelu_pool(p(out), p(rec), p(w), 2, 4, 4, 6, 2, 2, None, 0, None),                                           # C % 4
        lib.mt_mtcnn_prelu_pool(p(out), p(rec), p(w), 2, 4, 4, 8, 4, 2, None, 0, None),                                           # k
        lib.mt_mtcnn_prelu_pool(p(out), p(out), p(w), 2, 4, 4, 8, 2, 2, None, 0, None),                                           # in place
        lib.mt_mtcnn_score(p(out), 4, p(rec), p(win), p(cnt), 4, 8, 40, 40, 0.5, None),                                           # ldh
        lib.mt_mtcnn_finalize(p(rec), p(cnt), 5000, 8, 16, p(out), p(out), p(win), p(cnt), p(cnt), p(err), 16, None),             # N
        lib.mt_mtcnn_finalize(p(rec), p(cnt), 4, 8, 0, p(out), p(out), p(win), p(cnt), p(cnt), p(err), 16, None),                 # max_faces
    ]
    torch.cuda.synchronize()
    assert all(rc in (-1, -3) for rc in calls), calls
    assert lib.mt_last_error()
    assert rec.eq(2.0).all() and rec2.eq(2.0).all() and cnt.eq(3).all() and win.eq(3).all() and out.eq(2.0).all() and int(err.item()) == 0
