"""Face crops on the device (mintime_amd.face_crops, csrc/face_crops.hip) against the numpy restatements of tests/face_crops_ref.py
and the committed Pillow fixture.  Every comparison is exact: the kernels do Pillow's integer arithmetic, there is no tolerance."""
import os

import numpy as np
import pytest
import torch

import mintime_amd
from mintime_amd import face_crops as FC
from mintime_amd import lib
from tests import face_crops_ref as R
from tests import facenet_ref as FR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SQUARES = [(s, s) for s in (1, 2, 64, 75, 127, 128, 129, 255, 300)]
RECTANGLES = [(2, 3), (301, 299), (128, 200), (200, 128), (1000, 37), (37, 1000)]        # (height, width)
EXTREMES = [(4096, 5)]            # the longest side, as a tall strip: Image.resize's vertical-first order (the kernel's strip branch)
RAGGED = SQUARES + RECTANGLES + EXTREMES
_CACHE = {}


def source(h, w, seed=None):
    rng = np.random.default_rng(h * 10007 + w if seed is None else seed)
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def fixture():
    if "fx" not in _CACHE:
        _CACHE["fx"] = np.load(os.path.join(ROOT, "tests", "golden", "face_crops_pil.npz"))
    return _CACHE["fx"]


def ragged_run():
    """One run_ragged call over every listed size plus the fixture's sources -> (sources, device result on the host)."""
    if "ragged" not in _CACHE:
        fx = fixture()
        srcs = [source(h, w) for h, w in RAGGED] + [fx[f"src{i}"] for i in range(len(fx["shapes"]))]
        plan = FC.FaceCropPlan(len(srcs))
        res = plan.run_ragged([torch.from_numpy(s).cuda() for s in srcs])
        res.raise_on_error()
        assert res.crops.shape == (len(srcs), 128, 128, 3) and res.crops.dtype == torch.uint8
        _CACHE["ragged"] = (srcs, res.crops.cpu().numpy())
    return _CACHE["ragged"]


@pytest.mark.parametrize("h,w", RAGGED)
def test_ragged_entry_equals_the_restatement(h, w):
    srcs, got = ragged_run()
    i = RAGGED.index((h, w))
    assert np.array_equal(got[i], R.pil_resize_u8(srcs[i], 128, 128))


def test_ragged_entry_equals_the_pillow_fixture():
    srcs, got = ragged_run()
    fx = fixture()
    for i in range(len(fx["shapes"])):
        assert np.array_equal(got[len(RAGGED) + i], fx[f"out{i}"]), tuple(fx["shapes"][i])


def frames_case():
    """Two 360 x 480 frames and the box table, one plan.run -> everything on the host, plus the expected arrays."""
    if "frames" not in _CACHE:
        H, W = R.FRAME_H, R.FRAME_W
        frames = np.random.default_rng(5).integers(0, 256, (2, H, W, 3), dtype=np.uint8)
        boxes = np.array([b for _, b in R.BOXES], dtype=np.float32)
        T = len(boxes)
        index = (np.arange(T) % 2).astype(np.int32)
        want_rects = np.zeros((T, 4), dtype=np.int32)
        want_valid = np.zeros(T, dtype=np.uint8)
        want_crops = np.zeros((T, 128, 128, 3), dtype=np.uint8)
        for t, box in enumerate(boxes):
            x0, y0, w, h, v = R.crop_rect(tuple(float(b) for b in box), H, W)
            want_rects[t], want_valid[t] = (x0, y0, w, h), v
            if v:
                want_crops[t] = R.pil_resize_u8(frames[index[t], y0:y0 + h, x0:x0 + w], 128, 128)
        dev = (torch.from_numpy(frames).cuda(), torch.from_numpy(boxes).cuda(), torch.from_numpy(index).cuda())
        plan = FC.FaceCropPlan(T + 3)
        res = plan.run(*dev)
        _CACHE["frames"] = dict(dev=dev, plan=plan, res=res, crops=res.crops.cpu().numpy(), rects=res.rects.cpu().numpy(),
                                valid=res.valid.cpu().numpy(), want_rects=want_rects, want_valid=want_valid, want_crops=want_crops,
                                frames=frames, boxes=boxes, index=index)
    return _CACHE["frames"]


def test_frames_entry_rects_and_valid_equal_crop_rect():
    c = frames_case()
    assert c["want_valid"].sum() >= 12 and (c["want_valid"] == 0).sum() >= 4
    assert np.array_equal(c["valid"], c["want_valid"])
    assert np.array_equal(c["rects"], c["want_rects"]), [n for (n, _), a, b in zip(R.BOXES, c["rects"], c["want_rects"]) if tuple(a) != tuple(b)]


def test_frames_entry_crops_equal_the_restatement_of_the_host_slice():
    c = frames_case()
    bad = [n for (n, _), a, b in zip(R.BOXES, c["crops"], c["want_crops"]) if not np.array_equal(a, b)]
    assert bad == []
    for t in np.flatnonzero(c["want_valid"] == 0):
        assert not c["crops"][t].any()                     # an invalid face is all zeros


def test_invalid_boxes_are_counted_in_the_error_word():
    c = frames_case()
    n_invalid = int((c["want_valid"] == 0).sum())
    plan = FC.FaceCropPlan(len(R.BOXES))
    res = plan.run(*c["dev"])
    assert res.error_word() == (n_invalid, 0)
    with pytest.raises(lib.MintimeHipError, match=f"{n_invalid} invalid box"):
        res.raise_on_error()
    keep = torch.from_numpy(np.flatnonzero(c["want_valid"])).cuda()
    clean = FC.FaceCropPlan(len(R.BOXES))
    ok = clean.run(c["dev"][0], c["dev"][1][keep].contiguous(), c["dev"][2][keep].contiguous())
    assert ok.raise_on_error() is ok and bool(ok.valid.all())
    assert np.array_equal(ok.crops.cpu().numpy(), c["want_crops"][c["want_valid"] == 1])
    res2 = plan.run(*c["dev"])                             # sticky: the counter keeps counting
    assert res2.error_word() == (2 * n_invalid, 0)


def test_frame_index_outside_the_batch_is_invalid():
    c = frames_case()
    index = torch.from_numpy(c["index"]).clone()
    index[0], index[1] = 2, -1
    res = FC.FaceCropPlan(len(R.BOXES)).run(c["dev"][0], c["dev"][1], index.cuda())
    assert res.valid[:2].tolist() == [0, 0] and not res.crops[:2].any() and res.rects[:2].tolist() == [[0, 0, 0, 0]] * 2
    assert np.array_equal(res.crops[2:].cpu().numpy(), c["want_crops"][2:])
    assert res.error_word()[0] == int((c["want_valid"] == 0).sum()) + 2


def test_a_face_is_the_same_bytes_alone_and_inside_the_batch():
    c = frames_case()
    frames, boxes, index = c["dev"]
    plan = FC.FaceCropPlan(1)
    for t in (0, 5, 8, 12, 14):
        alone = plan.run(frames, boxes[t:t + 1].contiguous(), index[t:t + 1].contiguous())
        assert np.array_equal(alone.crops[0].cpu().numpy(), c["crops"][t]), R.BOXES[t][0]
        assert alone.rects[0].tolist() == c["rects"][t].tolist()
    srcs, got = ragged_run()
    for i in (RAGGED.index((300, 300)), RAGGED.index((4096, 5))):
        one = FC.resize_crops([torch.from_numpy(srcs[i]).cuda()])
        assert np.array_equal(one[0].cpu().numpy(), got[i])


@pytest.mark.parametrize("oh,ow", [(1, 1), (160, 96), (256, 256)])
def test_other_output_sizes(oh, ow):
    shapes = [(75, 75), (301, 299), (37, 300)]
    srcs = [source(h, w, seed=oh + h) for h, w in shapes]
    got = FC.resize_crops([torch.from_numpy(s).cuda() for s in srcs], (oh, ow)).cpu().numpy()
    assert got.shape == (3, oh, ow, 3)
    for s, g in zip(srcs, got):
        assert np.array_equal(g, R.pil_resize_u8(s, oh, ow)), s.shape


@pytest.mark.parametrize("oh,ow", [(128, 256), (1, 1), (2, 3)])
def test_one_output_row_over_several_fills_of_the_tile(oh, ow):
    """4096 x 64 (too wide for the tall-strip branch).  At 128 x 256 the tile holds 32 horizontal-pass rows and an output row has
    up to 65 taps; at 1 and 2 output rows there are 8193 and 4097 taps against the 2048 coefficients held at a time: both ways into
    the branch that keeps one row's sums in registers over several fills of the tile."""
    src = source(4096, 64, seed=oh * 1000 + ow)
    got = FC.resize_crops([torch.from_numpy(src).cuda()], (oh, ow)).cpu().numpy()
    assert np.array_equal(got[0], R.pil_resize_u8(src, oh, ow))


def test_window_side_limit_and_a_window_of_many_sub_bands():
    """4100 x 4100 frame: one box whose window is the whole frame (a side above 4096: invalid), one of 2332 x 2332 (18 source rows
    per output row: a band's rows do not fit the tile at once)."""
    H = W = 4100
    frames = torch.randint(0, 256, (1, H, W, 3), dtype=torch.uint8, device="cuda", generator=torch.Generator("cuda").manual_seed(3))
    boxes = np.array([(1.0, 1.0, 2049.0, 2049.0), (700.0, 700.0, 1400.0, 1400.0)], dtype=np.float32)
    want = [R.crop_rect(tuple(float(v) for v in b), H, W) for b in boxes]
    assert want[0] == (0, 0, 0, 0, 0) and want[1][2:] == (2332, 2332, 1)
    res = FC.FaceCropPlan(2).run(frames, torch.from_numpy(boxes).cuda(), torch.zeros(2, dtype=torch.int32, device="cuda"))
    assert res.valid.tolist() == [0, 1] and res.rects.tolist() == [list(w[:4]) for w in want]
    assert res.error_word() == (1, 0) and not res.crops[0].any()
    x0, y0, w, h, _ = want[1]
    window = frames[0, y0:y0 + h, x0:x0 + w].cpu().numpy()
    assert np.array_equal(res.crops[1].cpu().numpy(), R.pil_resize_u8(window, 128, 128))


def test_ragged_images_beyond_the_limit_are_refused_on_the_host():
    with pytest.raises(NotImplementedError, match=r"4097 x 2; sides of 1\.\.4096"):
        FC.resize_crops([torch.zeros(4097, 2, 3, dtype=torch.uint8, device="cuda")])
    with pytest.raises(ValueError, match=r"must be uint8 \[h, w, 3\]"):
        FC.resize_crops([torch.zeros(8, 8, 4, dtype=torch.uint8, device="cuda")])
    plan = FC.FaceCropPlan(2)
    with pytest.raises(ValueError, match="3 images, the plan was built for at most 2"):
        plan.run_ragged([torch.zeros(8, 8, 3, dtype=torch.uint8, device="cuda")] * 3)
    with pytest.raises(ValueError, match=r"frame_index must be contiguous int32 \[1\]"):
        plan.run(torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device="cuda"), torch.zeros(1, 4, device="cuda"),
                 torch.zeros(1, dtype=torch.int64, device="cuda"))


def embedder():
    if "model" not in _CACHE:
        m = mintime_amd.InceptionResnetV1()
        m.load_state_dict(FR.seeded_state(0))
        _CACHE["model"] = m.cuda().eval()
    return _CACHE["model"]


def test_crops_go_straight_into_the_embedder():
    c = frames_case()
    m = embedder()
    res = c["plan"].run(*c["dev"])
    direct = m.embed_crops(res.crops).clone()
    uploaded = m.embed_crops(torch.from_numpy(c["want_crops"]).cuda()).clone()
    assert direct.shape == (len(R.BOXES), 512) and torch.equal(direct, uploaded)
    sizes = res.rects[:, 2:].cpu().numpy()
    assert np.array_equal(sizes, c["want_rects"][:, 2:])


def test_second_run_at_the_same_shape_allocates_nothing():
    c = frames_case()
    plan = FC.FaceCropPlan(len(R.BOXES))
    first = plan.run(*c["dev"])
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats()["allocation.all.allocated"]
    again = plan.run(*c["dev"])
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == before
    assert again.crops.data_ptr() == first.crops.data_ptr() == plan.crops.data_ptr()
    assert np.array_equal(again.crops.cpu().numpy(), c["want_crops"])
