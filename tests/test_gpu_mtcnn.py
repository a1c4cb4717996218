"""The MTCNN detector end to end on the device: the committed case (tests/golden/mtcnn_case.npz: seeds, thresholds, the fp64
restatement's boxes per stage, its decision margin and the fp32 restatement's own error; tests/test_mtcnn_host.py asserts that the
margin is at least 50 times that error) -- counts and order equal at every stage, coordinates and probabilities within 50 times the
fp32 restatement's error; the package's containers; batch independence, bitwise; capacity overflow; no allocation after the first
call; refolding after load_state_dict; and Detections -> FaceCropPlan -> embedder."""
import numpy as np
import pytest
import torch

import mintime_amd
from mintime_amd import lib as L
from mintime_amd import mtcnn_engine as E
from tests import mtcnn_ref as R

pytestmark = pytest.mark.gpu
REC = E.REC


@pytest.fixture(scope="module")
def case():
    c = R.load_case()
    seed = int(c["seed"])
    c["frames"] = R.make_frames(seed, *(int(v) for v in c["shape"]))
    c["sd"] = {k: v.float() for k, v in R.healthy_weights(seed).items()}
    return c


def _detector(case, **kw):
    kw.setdefault("max_candidates", 128)
    kw.setdefault("max_faces", 32)
    kw.setdefault("max_refined", 32)
    d = mintime_amd.MTCNN(device="cuda", thresholds=[float(t) for t in case["thresholds"]], **kw)
    d.load_state_dict(case["sd"])
    return d


@pytest.fixture(scope="module")
def det(case):
    return _detector(case)


def test_detect_device_on_the_fixture_case(case, det):
    eng = det.engine()
    eng.debug = {}
    try:
        out = det.detect_device(case["frames"].cuda())
        out.raise_on_error()
        dbg = eng.debug
    finally:
        eng.debug = None
    N = case["frames"].shape[0]
    tol_c, tol_s = 50 * float(case["coord_err"]), 50 * float(case["score_err"])
    cand = dbg["cand"][1].cpu().reshape(N, -1)
    assert np.array_equal(cand.numpy(), case["cand_counts"])
    for st in ("stage1", "stage2", "stage3"):
        rec, cnt = (t.cpu() for t in dbg[st])
        assert cnt.tolist() == case[st + "_counts"].tolist(), st
        rows = torch.cat([rec[n, :int(cnt[n])] for n in range(N)])
        assert rows[:, 9].contiguous().view(torch.int32).tolist() == case[st + "_keys"].tolist(), st       # the same boxes in the same order
        dc = float((rows[:, :4].double() - torch.from_numpy(case[st + "_boxes"])).abs().max())
        print(f"{st}: {len(rows)} boxes, largest coordinate error {dc:.2e} (allowed {tol_c:.2e})")
        assert dc <= tol_c, st
        ds = float((rows[:, 4].double() - torch.from_numpy(case[st + "_scores"])).abs().max())
        print(f"{st}: largest probability error {ds:.2e} (allowed {tol_s:.2e})")
        assert ds <= tol_s, st
    n3 = int(case["stage3_counts"].sum())
    assert int(out.count.item()) == n3 and out.image_counts.tolist() == case["stage3_counts"].tolist()
    assert out.frame_index.tolist() == sum(([n] * int(k) for n, k in enumerate(case["stage3_counts"])), []) + [-1] * (32 - n3)
    rec, cnt = dbg["stage3"]
    rows = torch.cat([rec[n, :int(cnt[n])] for n in range(N)])
    assert torch.equal(out.boxes[:n3], rows[:, :4]) and torch.equal(out.probs[:n3], rows[:, 4])
    assert not out.boxes[n3:].any() and not out.probs[n3:].any()


def test_detect_returns_the_packages_containers(case, det):
    frames = case["frames"]
    blank = torch.full_like(frames[0], 127)
    boxes, probs = det.detect([frames[0].numpy(), blank.numpy(), frames[1].numpy()])
    assert isinstance(boxes, np.ndarray) and boxes.dtype == object and boxes.shape == (3,) and probs.shape == (3,)
    assert boxes[1] is None and probs[1] == [None]
    counts = case["stage3_counts"].tolist()
    assert [len(boxes[0]), len(boxes[2])] == counts and boxes[2].shape == (counts[1], 4) and probs[2].shape == (counts[1],)
    area = (boxes[2][:, 2] - boxes[2][:, 0]) * (boxes[2][:, 3] - boxes[2][:, 1])
    assert (np.diff(area) <= 0).all()                                           # select_largest
    assert np.allclose(sorted(probs[2].tolist()), sorted(case["stage3_scores"][counts[0]:].tolist()), rtol=0, atol=50 * float(case["score_err"]))
    # a single image gives its own entries; a 4-D tensor gives object arrays; fp32 frames holding integers are the same frames
    b1, p1 = det.detect(frames[1].numpy())
    assert np.array_equal(b1, boxes[2]) and np.array_equal(p1, probs[2])
    b4, p4 = det.detect(frames.float())
    assert b4.shape == (2,) and np.array_equal(b4[1], boxes[2]) and np.array_equal(b4[0], boxes[0])
    bb, pb = det.detect(blank.numpy())
    assert bb is None and pb == [None]
    # the reference's caller: FacenetDetector._detect_faces
    assert [b.tolist() if b is not None else None for b in boxes][1] is None
    with pytest.raises(ValueError, match="no pyramid level"):
        det.detect(np.zeros((19, 64, 3), np.uint8))


def test_a_frame_alone_equals_the_frame_in_a_batch_bitwise(case, det):
    frames = case["frames"].cuda()
    batch = det.detect_device(torch.cat([frames, frames[:1]]))
    b, p, idx = batch.boxes.clone(), batch.probs.clone(), batch.frame_index.clone()
    for n in (1, 0):
        alone = det.detect_device(frames[n:n + 1])
        k = int(alone.count.item())
        assert k == int(case["stage3_counts"][n])
        sel = idx == n
        assert torch.equal(alone.boxes[:k].view(torch.int32), b[sel].view(torch.int32)) and torch.equal(alone.probs[:k], p[sel])
    assert torch.equal(b[idx == 0], b[idx == 2])


def test_capacity_overflow_sets_the_error_word_and_stays_inside_the_buffers(case):
    small = _detector(case, max_candidates=8, max_refined=2, max_faces=2)
    out = small.detect_device(case["frames"].cuda())
    assert int(out.count.item()) <= 2 and out.boxes.shape == (2, 4)
    with pytest.raises(L.MintimeHipError, match="stage 1: candidates of one \\(image, level\\)"):
        out.raise_on_error()
    out.raise_on_error()                                                         # read and cleared
    # the appending kernel itself, between guard rows
    frames = case["frames"].cuda()
    N, H, W, _ = frames.shape
    hs, ws = E.level_size(H, W, 0.6)
    cap = 8
    guard = torch.full((N * cap + 16, REC), 4.0, device="cuda")
    rec = guard[8:8 + N * cap].view(N, cap, REC)
    cnt = torch.zeros(N, dtype=torch.int32, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    L.mt.mtcnn_pnet(frames, N, H, W, hs, ws, 0.6, 0, 1, small.engine().weights()["pnet"], float(case["thresholds"][0]), rec, cnt, cap, err, None,
                    None)
    assert cnt.tolist() == case["cand_counts"][:, 0].tolist() and int(cnt.min()) > cap and int(err.item()) == 1
    assert guard[:8].eq(4.0).all() and guard[8 + N * cap:].eq(4.0).all() and not rec.eq(4.0).any()
    # Detections with fewer rows than faces: mt_mtcnn_finalize between guard values
    rec = torch.arange(2 * 4 * REC, dtype=torch.float32, device="cuda").view(2, 4, REC)
    counts = torch.tensor([1, 9], dtype=torch.int32, device="cuda")             # the second list overflowed its own capacity of 4
    guard = torch.full((3 * 4 + 3 + 16,), 4.0, device="cuda")
    boxes, probs = guard[8:20].view(3, 4), guard[20:23]
    fi = torch.full((3 + 8,), -9, dtype=torch.int32, device="cuda")
    total, per = torch.zeros((), dtype=torch.int32, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
    err.zero_()
    L.mt.mtcnn_finalize(rec, counts, 2, 4, 3, boxes, probs, fi[4:7], total, per, err, 16)
    assert int(total.item()) == 3 and per.tolist() == [1, 2] and fi.tolist() == [-9] * 4 + [0, 1, 1] + [-9] * 4 and int(err.item()) == 16
    assert torch.equal(boxes, torch.stack([rec[0, 0, :4], rec[1, 0, :4], rec[1, 1, :4]])) and probs.tolist() == [4.0, 52.0, 64.0]
    assert guard[:8].eq(4.0).all() and guard[23:].eq(4.0).all()


def test_no_allocation_after_the_first_call_at_a_shape(case, det):
    frames = case["frames"].cuda()
    det.detect_device(frames)
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats()["allocation.all.allocated"]
    a = det.detect_device(frames)
    first = a.boxes.clone()
    after_clone = torch.cuda.memory_stats()["allocation.all.allocated"]
    b = det.detect_device(frames)
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == after_clone == before + 1
    assert a.boxes.data_ptr() == b.boxes.data_ptr() and torch.equal(first, b.boxes)


def test_load_state_dict_refolds_the_weights(case):
    frames = case["frames"].cuda()
    d = _detector(case)
    ref = d.detect_device(frames).boxes.clone()
    other = {k: v.float() for k, v in R.healthy_weights(int(case["seed"]) + 1).items()}
    d.load_state_dict(other)
    got = d.detect_device(frames)
    fresh = mintime_amd.MTCNN(device="cuda", thresholds=d.thresholds, max_candidates=128, max_refined=32, max_faces=32)
    fresh.load_state_dict(other)
    want = fresh.detect_device(frames)
    assert torch.equal(got.boxes, want.boxes) and torch.equal(got.image_counts, want.image_counts) and not torch.equal(got.boxes, ref)
    with torch.no_grad():
        d.pnet.conv4_1.bias.add_(torch.tensor([30.0, -30.0], device="cuda"))      # an in-place edit: nothing passes stage 1 any more
    assert int(d.detect_device(frames).count.item()) == 0


def test_detections_chain_into_the_crop_plan_and_the_embedder(case, det):
    frames = case["frames"].cuda()
    big = torch.nn.functional.interpolate(frames.permute(0, 3, 1, 2).float(), scale_factor=2, mode="nearest").permute(0, 2, 3, 1)
    big = big.to(torch.uint8).contiguous()                                       # the crop rule takes half-resolution boxes
    out = det.detect_device(frames)
    n = int(out.count.item())
    plan = mintime_amd.FaceCropPlan(max_faces=out.boxes.shape[0])
    crops = plan.run(big, out.boxes, out.frame_index)                            # at capacity rows: the unused ones come out invalid
    invalid, bits = crops.error_word()
    assert invalid == out.boxes.shape[0] - n and bits == 0 and crops.valid[:n].all() and not crops.valid[n:].any()
    embedder = mintime_amd.InceptionResnetV1(device="cuda").eval()
    emb = embedder.embed_crops(crops.crops).clone()
    # the host-side chain on the same boxes
    boxes_h, idx_h = out.boxes[:n].cpu(), out.frame_index[:n].cpu()
    plan2 = mintime_amd.FaceCropPlan(max_faces=n)
    crops2 = plan2.run(big, boxes_h.cuda(), idx_h.cuda())
    crops2.raise_on_error()
    assert torch.equal(crops2.crops, crops.crops[:n])
    emb2 = embedder.embed_crops(crops2.crops)
    assert torch.equal(emb2, emb[:n]) and torch.isfinite(emb2).all()
