"""Face crops for the embedder, cut and resized on the device: from the detector's boxes (or from ready crops of any size) to the
stacked uint8 `[T, 128, 128, 3]` array `InceptionResnetV1.embed_crops` takes.

The reference does this on the host, one face at a time: the crop rule of predict.py:103-140 (the same lines are
preprocessing/extract_crops.py:75-113) -- double the box, pad it by a third, square it, clamp it to the frame, trim it back towards
square -- then `preprocess_images` (preprocessing/utils.py:32-34; predict.py:151, preprocessing/cluster_faces.py:85): torchvision
`Resize([128, 128])` of a PIL image, which is Pillow's antialiased 8-bit bilinear `Image.resize`, then `np.stack` and an upload.  Here
it is two launches with no host read (csrc/face_crops.hip; both rules are stated in include/mintime_hip.h):

  * the windows are computed from the boxes in integers, one thread per face; a box whose window is empty, would wrap around as a
    Python slice, has a side above 4096 pixels or names a frame outside the batch is invalid: its crop is all zeros, `valid` is 0 and a
    sticky device counter goes up (read only by `FaceCrops.raise_on_error`, which synchronises);
  * the resize is Pillow's arithmetic exactly -- double-precision weights without contraction, 22-bit integer coefficients, a
    horizontal pass into uint8, a vertical pass over that -- so the bytes are the ones `Image.resize((128, 128), BILINEAR)` returns.

Not covered: detection (MTCNN), the 224 x 224 model-side crops (albumentations / cv2), video decoding."""
from typing import List, Sequence, Tuple

import torch

from . import lib as L

MAX_SIDE = 4096          # longest source window side (csrc/face_crops.hip)
MAX_OUT = 256            # longest output side
MAX_FACES = 65535        # faces of one launch (grid.y)


def _check_out_size(out_size) -> Tuple[int, int]:
    try:
        oh, ow = (int(v) for v in out_size)
    except (TypeError, ValueError):
        raise ValueError(f"out_size must be (height, width), got {out_size!r}") from None
    if not (1 <= oh <= MAX_OUT and 1 <= ow <= MAX_OUT):
        raise NotImplementedError(f"output size {oh} x {ow}: sides of 1..{MAX_OUT} are built")
    return oh, ow


def _check_max_faces(max_faces) -> int:
    if int(max_faces) < 1:
        raise ValueError(f"max_faces = {max_faces}: at least one face")
    if int(max_faces) > MAX_FACES:
        raise NotImplementedError(f"max_faces = {max_faces}: one launch takes at most {MAX_FACES} faces")
    return int(max_faces)


def _check_frames(frames, boxes, frame_index, max_faces):
    """-> (N, H, W, T) of a frames call, or raises before anything is launched."""
    for name, t in (("frames", frames), ("boxes", boxes), ("frame_index", frame_index)):
        if not (torch.is_tensor(t) and t.is_cuda):
            raise ValueError(f"face crops: {name} must be a tensor on the device (there is no CPU path)")
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or 0 in frames.shape:
        raise ValueError(f"face crops: frames must be uint8 [N, H, W, 3], got {frames.dtype} {tuple(frames.shape)}")
    if not frames.is_contiguous():
        raise ValueError("face crops: frames must be contiguous")
    if boxes.dtype != torch.float32 or boxes.dim() != 2 or boxes.shape[1] != 4 or not boxes.is_contiguous():
        raise ValueError(f"face crops: boxes must be contiguous fp32 [T, 4], got {boxes.dtype} {tuple(boxes.shape)}")
    T = boxes.shape[0]
    if frame_index.dtype != torch.int32 or tuple(frame_index.shape) != (T,) or not frame_index.is_contiguous():
        raise ValueError(f"face crops: frame_index must be contiguous int32 [{T}], got {frame_index.dtype} {tuple(frame_index.shape)}")
    if T > max_faces:
        raise ValueError(f"face crops: {T} boxes, the plan was built for at most {max_faces}")
    N, H, W, _ = frames.shape
    if max(N, H, W) >= 1 << 31:
        raise NotImplementedError(f"face crops: frames {tuple(frames.shape)}: the sizes are 32-bit counts")
    return N, H, W, T


def _check_images(images, max_faces) -> List[Tuple[int, int]]:
    """-> [(h, w)] of a ragged call, or raises before anything is launched."""
    if not isinstance(images, (list, tuple)) or not images:
        raise ValueError("face crops: images must be a non-empty list of uint8 [h, w, 3] device tensors")
    if len(images) > max_faces:
        raise ValueError(f"face crops: {len(images)} images, the plan was built for at most {max_faces}")
    sizes = []
    for i, im in enumerate(images):
        if not (torch.is_tensor(im) and im.is_cuda):
            raise ValueError(f"face crops: image {i} must be a tensor on the device (there is no CPU path)")
        if im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3 or 0 in im.shape:
            raise ValueError(f"face crops: image {i} must be uint8 [h, w, 3], got {im.dtype} {tuple(im.shape)}")
        if max(im.shape[0], im.shape[1]) > MAX_SIDE:
            raise NotImplementedError(f"face crops: image {i} is {im.shape[0]} x {im.shape[1]}; sides of 1..{MAX_SIDE} are built")
        sizes.append((int(im.shape[0]), int(im.shape[1])))
    return sizes


class FaceCrops:
    """crops [T, OH, OW, 3] uint8, and for a frames call rects [T, 4] int32 (x0, y0, w, h; zeros where invalid) and valid [T] uint8
    (None for ready crops): device tensors that belong to the plan that produced them and are overwritten by its next run."""

    def __init__(self, crops, rects, valid, err):
        self.crops, self.rects, self.valid = crops, rects, valid
        self._err = err

    def error_word(self) -> Tuple[int, int]:
        """(invalid boxes counted so far by the plan, table-error bits); synchronises."""
        e = self._err.cpu()            # (a synchronising copy on the current stream: the crops are complete after it)
        return int(e[0]), int(e[1])

    def raise_on_error(self):
        """Synchronises; raises if any box of this plan has been invalid or a window lay outside its source."""
        invalid, bits = self.error_word()
        if invalid or bits:
            what = []
            if invalid:
                what.append(f"{invalid} invalid box(es): empty window, negative far end, side above {MAX_SIDE} or frame outside the batch "
                            "(their crops are zeros, valid = 0)")
            if bits:
                what.append("a window outside its source or above the size the launch was sized for (its crop is zeros)")
            raise L.MintimeHipError("face crops: " + "; ".join(what))
        return self


class FaceCropPlan:
    """The crop-and-resize of up to `max_faces` faces to `out_size` = (height, width).

        plan = FaceCropPlan(max_faces=256)
        faces = plan.run(frames, boxes, frame_index)        # two launches on the current stream, nothing read back
        emb = embedder.embed_crops(faces.crops)             # [T, 512]
        sizes = faces.rects[:, 2:]                          # (w, h) of every face, for sequence.Identity

    The constructor owns every buffer; `run` only launches and allocates nothing."""

    def __init__(self, max_faces: int, out_size: Sequence[int] = (128, 128), device="cuda"):
        self.max_faces = _check_max_faces(max_faces)
        self.out_size = _check_out_size(out_size)
        dev = torch.device(device)
        if dev.type != "cuda":
            raise ValueError("FaceCropPlan lives on the device (there is no CPU path)")
        self.device = dev
        oh, ow = self.out_size
        self.crops = torch.empty(self.max_faces, oh, ow, 3, dtype=torch.uint8, device=dev)
        self.rects = torch.empty(self.max_faces, 4, dtype=torch.int32, device=dev)
        self.valid = torch.empty(self.max_faces, dtype=torch.uint8, device=dev)
        self.err = L.zeros(2, torch.int32, dev)
        self._table = None          # [max_faces, 4] int64 and the packed bytes of the ragged entry, made on its first use
        self._packed = None

    @torch.no_grad()
    def run(self, frames, boxes, frame_index) -> FaceCrops:
        """frames [N, H, W, 3] uint8, boxes [T, 4] fp32 (xmin, ymin, xmax, ymax as the detector returns them: half-resolution
        coordinates), frame_index [T] int32, all on the device -> FaceCrops (views of this plan's buffers)."""
        N, H, W, T = _check_frames(frames, boxes, frame_index, self.max_faces)
        oh, ow = self.out_size
        crops, rects, valid = self.crops[:T], self.rects[:T], self.valid[:T]
        if T:
            L.mt.face_rects(boxes, frame_index, T, N, H, W, rects, valid, self.err)
            L.mt.crop_resize_u8(frames, frames.numel(), N, H, W, rects, frame_index, valid, None, T, min(W, MAX_SIDE), oh, ow, crops,
                                self.err)
        return FaceCrops(crops, rects, valid, self.err)

    @torch.no_grad()
    def run_ragged(self, images) -> FaceCrops:
        """images: list of uint8 [h, w, 3] device tensors of any sizes (crops loaded from files) -> FaceCrops with rects = valid =
        None.  One concatenation into the plan's byte buffer, one table upload, one launch.  Unlike `run` this entry allocates on every
        call: the pinned host copy of the offset table, and a contiguous copy of any image that is not contiguous."""
        sizes = _check_images(images, self.max_faces)
        oh, ow = self.out_size
        T = len(images)
        rows, off = [], 0
        for h, w in sizes:
            rows.append((off, 3 * w, w, h))
            off += 3 * w * h
        if self._table is None:
            self._table = torch.empty(self.max_faces, 4, dtype=torch.int64, device=self.device)
        if self._packed is None or self._packed.numel() < off:
            self._packed = torch.empty(off, dtype=torch.uint8, device=self.device)
        packed, table = self._packed[:off], self._table[:T]
        torch.cat([im.contiguous().reshape(-1) for im in images], out=packed)
        table.copy_(torch.tensor(rows, dtype=torch.int64).pin_memory(), non_blocking=True)
        crops = self.crops[:T]
        L.mt.crop_resize_u8(packed, off, 0, 0, 0, None, None, None, table, T, max(w for _, w in sizes), oh, ow, crops, self.err)
        return FaceCrops(crops, None, None, self.err)


def resize_crops(images, out_size=(128, 128)):
    """`preprocess_images` for a list of uint8 [h, w, 3] device tensors -> [T, OH, OW, 3] uint8 (a fresh plan's buffer)."""
    out_size = _check_out_size(out_size)
    _check_images(images, MAX_FACES)
    return FaceCropPlan(len(images), out_size, images[0].device).run_ragged(images).crops
