"""Face crops for the embedder, on a machine without a device: the numpy restatements of tests/face_crops_ref.py against Pillow
itself (the committed fixture, and the installed Pillow where there is one) and against the reference's crop arithmetic run on a
coordinate-coded frame; the new entry points in the header and the binding table; argument errors raised before any launch."""
import os
import re

import numpy as np
import pytest
import torch

import mintime_amd
from mintime_amd import face_crops as FC
from mintime_amd import lib
from tests import face_crops_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECT_SOURCES = [(2, 3), (301, 299), (513, 640), (128, 200), (200, 128), (1000, 37), (255, 256), (383, 385)]      # (height, width)
TALL_STRIPS = [(600, 5), (257, 2), (4096, 5), (500, 5), (501, 5), (300, 3), (301, 3)]      # around Image.resize's height > 100 width


def fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "face_crops_pil.npz"))


def sources(h, w, seed):
    """Random content and a 0 / 255 checkerboard (every sum of coefficients meets the clip) of one size."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w]
    board = np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8), board


def test_restatement_equals_the_pillow_fixture():
    fx = fixture()
    assert [tuple(s) for s in fx["shapes"]] == [(1, 1), (2, 3), (75, 75), (129, 127), (37, 300), (300, 2)]
    for i, (h, w) in enumerate(fx["shapes"]):
        src = fx[f"src{i}"]
        assert src.shape == (h, w, 3)
        assert np.array_equal(R.pil_resize_u8(src, 128, 128), fx[f"out{i}"]), (h, w, str(fx["pillow_version"]))


def _against_pillow(Image, src, oh, ow):
    want = np.asarray(Image.fromarray(src).resize((ow, oh), Image.BILINEAR))
    got = R.pil_resize_u8(src, oh, ow)
    assert np.array_equal(got, want), (src.shape, oh, ow, int(np.abs(got.astype(int) - want).max()))


def test_restatement_equals_pillow_on_every_square_side_to_260():
    Image = pytest.importorskip("PIL.Image")
    for side in range(1, 261):
        for src in sources(side, side, side):
            _against_pillow(Image, src, 128, 128)


@pytest.mark.parametrize("h,w", RECT_SOURCES)
def test_restatement_equals_pillow_on_rectangles(h, w):
    Image = pytest.importorskip("PIL.Image")
    for src in sources(h, w, 1000 + h):
        _against_pillow(Image, src, 128, 128)


@pytest.mark.parametrize("oh,ow", [(1, 1), (96, 160), (256, 256)])
def test_restatement_equals_pillow_at_other_output_sizes(oh, ow):
    Image = pytest.importorskip("PIL.Image")
    for h, w in ((75, 75), (301, 299), (37, 300)):
        for src in sources(h, w, 2000 + h):
            _against_pillow(Image, src, oh, ow)


def test_tall_strips_follow_the_installed_pillow():
    """Image.resize (the Python method, as of Pillow 12.2.0) shortens a source more than 100 times as tall as wide BEFORE widening it;
    the restatement and the kernel do the same, and the fixture's 300 x 2 source pins that order where no Pillow is installed.  The
    two orders give different bytes: a Pillow release without that branch fails here."""
    Image = pytest.importorskip("PIL.Image")
    for h, w in TALL_STRIPS:
        for src in sources(h, w, 3000 + h):
            _against_pillow(Image, src, 128, 128)
    assert R.vertical_first(501, 5, 128) and not R.vertical_first(500, 5, 128) and not R.vertical_first(501, 5, 501)


@pytest.mark.parametrize("oh,ow", [(1, 1), (2, 3), (128, 256)])
def test_restatement_equals_pillow_where_one_output_row_has_thousands_of_taps(oh, ow):
    """4096 x 64 (not a tall strip): 8193 / 4097 taps per output row at 1 / 2 rows, 65 at 128 -- the sizes at which the kernel
    fills its LDS tile several times for one output row (tests/test_gpu_face_crops.py)."""
    Image = pytest.importorskip("PIL.Image")
    for src in sources(4096, 64, 4000 + oh):
        _against_pillow(Image, src, oh, ow)


def reference_window(box, frame):
    """What the reference's lines do to one box, by doing it: the same integer steps and the same numpy slices on a frame whose
    pixel (y, x) holds (y, x).  -> (x0, y0, w, h), or None where the crop comes out empty."""
    left, top, right, bottom = [int(v * 2) for v in box]
    bw, bh = right - left, bottom - top
    pad_y, pad_x = bh // 3, bw // 3
    tall = (bottom + pad_y) - max(top - pad_y, 0)
    wide = (right + pad_x) - max(left - pad_x, 0)
    if tall > wide:
        pad_y -= int((tall - wide) / 2)
    else:
        pad_x -= int((wide - tall) / 2)
    cut = frame[max(top - pad_y, 0):bottom + pad_y, max(left - pad_x, 0):right + pad_x]
    rows, cols = cut.shape[:2]
    if rows > cols:
        d = int((rows - cols) / 2)
        cut = cut[d:-d, :] if d > 0 else cut[1:, :]
    elif rows < cols:
        d = int((cols - rows) / 2)
        cut = cut[:, d:-d] if d > 0 else cut[:, :-1]
    if cut.size == 0:
        return None
    y0, x0 = (int(v) for v in cut[0, 0])
    y1, x1 = (int(v) for v in cut[-1, -1])
    assert (y1 - y0 + 1, x1 - x0 + 1) == cut.shape[:2]
    return x0, y0, cut.shape[1], cut.shape[0]


def coded_frame(H, W):
    yy, xx = np.mgrid[:H, :W]
    return np.stack([yy, xx], axis=2).astype(np.int32)


def test_crop_rect_equals_the_reference_lines_on_the_box_table():
    frame = coded_frame(R.FRAME_H, R.FRAME_W)
    seen_valid = seen_invalid = 0
    for name, box in R.BOXES:
        x0, y0, w, h, valid = R.crop_rect(box, R.FRAME_H, R.FRAME_W)
        if not all(np.isfinite(box)):
            assert valid == 0, name
            continue
        want = reference_window(tuple(float(np.float32(b)) for b in box), frame)
        if valid:
            assert want == (x0, y0, w, h), (name, want, (x0, y0, w, h))
            seen_valid += 1
        else:
            assert (x0, y0, w, h) == (0, 0, 0, 0), name
            seen_invalid += 1
            if name != "negative far end":                   # (there the reference's slice wraps around to a window of its own)
                assert want is None, (name, want)
    assert seen_valid >= 12 and seen_invalid >= 3
    by_name = {n: R.crop_rect(b, R.FRAME_H, R.FRAME_W) for n, b in R.BOXES}
    assert by_name["one row too many"][1] == by_name["interior"][1] + 1            # h - w == 1: the first row goes
    assert by_name["negative near corner"][2:4] == (83, 84)                        # one off square stays one off
    assert by_name["one pixel wide"][2:4] == (1, 1)


def test_crop_rect_equals_the_reference_lines_on_random_boxes():
    H, W = 97, 131
    frame = coded_frame(H, W)
    rng = np.random.default_rng(7)
    agree = 0
    for _ in range(3000):
        a = rng.uniform(-20, 80, size=2).astype(np.float32)
        size = rng.uniform(0, 60, size=2).astype(np.float32) * rng.choice([1.0, 0.1], size=2).astype(np.float32)
        box = (float(a[0]), float(a[1]), float(a[0] + size[0]), float(a[1] + size[1]))
        x0, y0, w, h, valid = R.crop_rect(box, H, W)
        if valid:
            assert reference_window(box, frame) == (x0, y0, w, h), box
            agree += 1
    assert agree > 1000              # (a third of the boxes start outside the 97 x 131 frame or left of it)


def test_crop_rect_side_limit():
    assert R.crop_rect((0.0, 0.0, 2500.0, 2500.0), 5000, 5000) == (0, 0, 0, 0, 0)
    assert R.crop_rect((0.0, 0.0, 2500.0, 2500.0), 4096, 4096) == (0, 0, 4096, 4096, 1)


def test_abi_declares_the_new_entry_points_at_version_123():
    with open(os.path.join(ROOT, "include", "mintime_hip.h")) as fh:
        header = fh.read()
    assert int(re.search(r"#define MT_VERSION (\d+)", header).group(1)) == lib.ABI_VERSION == 123
    for name in ("mt_face_rects", "mt_crop_resize_u8"):
        assert re.search(r"^int %s\(" % name, header, flags=re.M), name
        assert name in lib.LAUNCHES
    handle = lib.get()
    assert handle.mt_version() == 123
    assert callable(lib.mt.face_rects) and callable(lib.mt.crop_resize_u8)
    assert mintime_amd.FaceCropPlan is FC.FaceCropPlan and mintime_amd.resize_crops is FC.resize_crops


def test_entry_points_refuse_bad_arguments_before_launching():
    with pytest.raises(lib.MintimeHipError, match=r"mt_face_rects failed .*T = 1, N = 0"):
        lib.mt.face_rects(None, None, 1, 0, 8, 8, None, None, None, None)
    with pytest.raises(lib.MintimeHipError, match=r"mt_face_rects failed .*null pointer"):
        lib.mt.face_rects(None, None, 1, 1, 8, 8, None, None, None, None)
    with pytest.raises(lib.MintimeHipError, match=r"mt_crop_resize_u8 failed .*output 257 x 128"):
        lib.mt.crop_resize_u8(None, 0, 1, 8, 8, None, None, None, None, 1, 8, 257, 128, None, None, None)
    with pytest.raises(lib.MintimeHipError, match=r"mt_crop_resize_u8 failed .*max_w = 4097"):
        lib.mt.crop_resize_u8(None, 0, 1, 8, 8, None, None, None, None, 1, 4097, 128, 128, None, None, None)
    with pytest.raises(lib.MintimeHipError, match=r"mt_crop_resize_u8 failed .*exceed src_bytes"):
        lib.mt.crop_resize_u8(None, 10, 1, 8, 8, None, None, None, None, 1, 8, 128, 128, None, None, None)


def test_argument_errors_are_raised_without_a_device():
    with pytest.raises(ValueError, match="at least one face"):
        FC.FaceCropPlan(0)
    with pytest.raises(NotImplementedError, match="at most 65535"):
        FC.FaceCropPlan(70000)
    with pytest.raises(NotImplementedError, match=r"sides of 1\.\.256"):
        FC.FaceCropPlan(4, (128, 257))
    with pytest.raises(NotImplementedError, match=r"sides of 1\.\.256"):
        FC.FaceCropPlan(4, (0, 128))
    with pytest.raises(ValueError, match="height, width"):
        FC.FaceCropPlan(4, 128)
    with pytest.raises(ValueError, match="no CPU path"):
        FC.FaceCropPlan(4, device="cpu")
    cpu = torch.zeros(5, 4, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="image 0 must be a tensor on the device"):
        FC.resize_crops([cpu])
    with pytest.raises(ValueError, match="non-empty list"):
        FC.resize_crops([])
    with pytest.raises(ValueError, match="frames must be a tensor on the device"):
        FC._check_frames(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), torch.zeros(1, 4), torch.zeros(1, dtype=torch.int32), 4)
