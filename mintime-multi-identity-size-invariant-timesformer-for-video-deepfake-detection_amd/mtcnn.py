"""MTCNN: the face detector in front of the crops, the embedder and the clustering, inference only, on the HIP path
(mtcnn_engine.py, csrc/mtcnn.hip).

The reference takes `facenet_pytorch.models.mtcnn.MTCNN(device, thresholds=[0.85, 0.95, 0.95], margin=0)` and calls
`.detect(frames, landmarks=False)` on batches of 32 equal-size frames (preprocessing/face_detector.py:38-56).  This module rebuilds
that detector from its published source, with the package's module and parameter names, so its state dicts load:

    from mintime_amd import MTCNN
    detector = MTCNN(device='cuda', thresholds=[0.85, 0.95, 0.95], margin=0, weights_path='facenet_weights/')
    batch_boxes, batch_probs = detector.detect(frames)           # the package's containers (one host read)
    det = detector.detect_device(frames_u8)                      # Detections: device tensors, no host read

UNCHECKED against facenet_pytorch: the package is not available where this was written, so the three networks, the key names
(tests/golden/mtcnn_manifest.json) and the post-processing (include/mintime_hip.h states it in full) are restated by hand from its
published source and have not been compared with the package or a real checkpoint.

Defined deviations from the package: (a) equal scores in an NMS order are broken by the candidate's (image, level, y, x) ascending;
(b) NMS runs per image on the coordinates themselves; (c) a stage-2/3 window without a pixel is dropped; (d) the lists have fixed
capacities (`max_candidates` per (image, level) and per image in stage 1, `max_refined` per image after R-Net, `max_faces` per batch)
and an overflow is reported by `Detections.raise_on_error()`.  INTEGRATION.md section 1 gives the window of each.

Not covered: landmarks (`dense6_3` is held for the state dict and never launched), `forward` / `extract` (crop saving), training,
downloading weights.  There is no CPU path."""
import os

import numpy as np
import torch
from torch import nn

from . import lib as L
from . import mtcnn_engine as E
from .mtcnn_engine import Detections  # noqa: F401


def _never(self, *a, **k):
    raise L.MintimeHipError("MTCNN submodules only hold weights: call detect / detect_device (the HIP engine runs the layers)")


class PNet(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 10, kernel_size=3)
        self.prelu1 = nn.PReLU(10)
        self.pool1 = nn.MaxPool2d(2, 2, ceil_mode=True)
        self.conv2 = nn.Conv2d(10, 16, kernel_size=3)
        self.prelu2 = nn.PReLU(16)
        self.conv3 = nn.Conv2d(16, 32, kernel_size=3)
        self.prelu3 = nn.PReLU(32)
        self.conv4_1 = nn.Conv2d(32, 2, kernel_size=1)
        self.softmax4_1 = nn.Softmax(dim=1)
        self.conv4_2 = nn.Conv2d(32, 4, kernel_size=1)

    forward = _never


class RNet(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 28, kernel_size=3)
        self.prelu1 = nn.PReLU(28)
        self.pool1 = nn.MaxPool2d(3, 2, ceil_mode=True)
        self.conv2 = nn.Conv2d(28, 48, kernel_size=3)
        self.prelu2 = nn.PReLU(48)
        self.pool2 = nn.MaxPool2d(3, 2, ceil_mode=True)
        self.conv3 = nn.Conv2d(48, 64, kernel_size=2)
        self.prelu3 = nn.PReLU(64)
        self.dense4 = nn.Linear(576, 128)
        self.prelu4 = nn.PReLU(128)
        self.dense5_1 = nn.Linear(128, 2)
        self.softmax5_1 = nn.Softmax(dim=1)
        self.dense5_2 = nn.Linear(128, 4)

    forward = _never


class ONet(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 32, kernel_size=3)
        self.prelu1 = nn.PReLU(32)
        self.pool1 = nn.MaxPool2d(3, 2, ceil_mode=True)
        self.conv2 = nn.Conv2d(32, 64, kernel_size=3)
        self.prelu2 = nn.PReLU(64)
        self.pool2 = nn.MaxPool2d(3, 2, ceil_mode=True)
        self.conv3 = nn.Conv2d(64, 64, kernel_size=3)
        self.prelu3 = nn.PReLU(64)
        self.pool3 = nn.MaxPool2d(2, 2, ceil_mode=True)
        self.conv4 = nn.Conv2d(64, 128, kernel_size=2)
        self.prelu4 = nn.PReLU(128)
        self.dense5 = nn.Linear(1152, 256)
        self.prelu5 = nn.PReLU(256)
        self.dense6_1 = nn.Linear(256, 2)
        self.softmax6_1 = nn.Softmax(dim=1)
        self.dense6_2 = nn.Linear(256, 4)
        self.dense6_3 = nn.Linear(256, 10)                 # landmarks: held for the checkpoint's keys, never launched

    forward = _never


def _to_uint8_array(img):
    """One image of the package's kinds (PIL image, array, tensor; [H, W, 3]) as a host uint8-valued array."""
    if torch.is_tensor(img):
        return img.detach().cpu().numpy()
    return np.asarray(img)


class MTCNN(nn.Module):
    """facenet_pytorch's constructor signature plus `weights_path` (a directory holding pnet.pt, rnet.pt and onet.pt, or one state
    dict with `pnet.` / `rnet.` / `onet.` keys; nothing is downloaded), `max_candidates` (capacity of every stage-1 list, per
    (image, level) and per image = the rows R-Net runs per image; at most 1024), `max_refined` (boxes per image that R-Net may keep =
    the rows O-Net runs per image) and `max_faces` (rows of `Detections`, for the whole batch)."""

    def __init__(self, image_size=160, margin=0, min_face_size=20, thresholds=[0.6, 0.7, 0.7], factor=0.709, post_process=True,
                 select_largest=True, selection_method=None, keep_all=False, device=None, weights_path=None, max_candidates=256,
                 max_refined=64, max_faces=256):
        super().__init__()
        if len(thresholds) != 3:
            raise ValueError(f"MTCNN: thresholds = {thresholds!r}: one per stage")
        if not 1 <= int(max_candidates) <= E.MAX_LIST:
            raise ValueError(f"MTCNN: max_candidates = {max_candidates}: 1..{E.MAX_LIST} (one wavefront sorts a list)")
        if not 1 <= int(max_refined) <= int(max_candidates):
            raise ValueError(f"MTCNN: max_refined = {max_refined}: 1..max_candidates")
        if int(max_faces) < 1:
            raise ValueError(f"MTCNN: max_faces = {max_faces}: at least one face")
        if not (min_face_size > 0 and 0 < factor < 1):
            raise ValueError(f"MTCNN: min_face_size = {min_face_size}, factor = {factor}")
        self.image_size, self.margin, self.min_face_size = image_size, margin, min_face_size
        self.thresholds, self.factor, self.post_process = [float(t) for t in thresholds], factor, post_process
        self.select_largest, self.keep_all = select_largest, keep_all
        self.selection_method = selection_method
        self.max_candidates, self.max_refined, self.max_faces = int(max_candidates), int(max_refined), int(max_faces)
        self.pnet, self.rnet, self.onet = PNet(), RNet(), ONet()
        if weights_path is not None:
            if os.path.isdir(weights_path):
                for name in ("pnet", "rnet", "onet"):
                    getattr(self, name).load_state_dict(torch.load(os.path.join(weights_path, name + ".pt"), map_location="cpu"))
            else:
                self.load_state_dict(torch.load(weights_path, map_location="cpu"))
        self.device = torch.device("cpu")
        if device is not None:
            self.device = torch.device(device)
            self.to(self.device)
        if not self.selection_method:
            self.selection_method = "largest" if self.select_largest else "probability"
        self._engine = None

    def engine(self):
        if self.__dict__.get("_engine") is None:
            self.__dict__["_engine"] = E.Engine(self)
        return self.__dict__["_engine"]

    def __deepcopy__(self, memo):
        import copy
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            new.__dict__[k] = None if k == "_engine" else copy.deepcopy(v, memo)
        return new

    def __getstate__(self):
        d = dict(self.__dict__)
        d["_engine"] = None
        return d

    def forward(self, img, save_path=None, return_prob=False):
        raise NotImplementedError("MTCNN.forward (cropped, saved face tensors) is not on the HIP path: call detect / detect_device and "
                                  "FaceCropPlan.run")

    def extract(self, img, batch_boxes, save_path):
        raise NotImplementedError("MTCNN.extract (crop saving) is not on the HIP path: FaceCropPlan.run cuts the crops on the device")

    def check_size(self, H, W):
        if min(H, W) * 12.0 / self.min_face_size < 12:
            raise ValueError(f"MTCNN: {H} x {W} frames hold no pyramid level at min_face_size = {self.min_face_size}")

    def detect_device(self, frames) -> Detections:
        """frames: [N, H, W, 3] uint8 on the device, or fp32 holding integer values -> Detections (buffers of this module).
        No host read; `Detections.raise_on_error()` is the only synchronising call."""
        if not torch.is_tensor(frames) or not frames.is_cuda:
            raise L.MintimeHipError("MTCNN (MI355X build) needs device tensors; frames is on the CPU and there is no CPU path")
        if frames.dim() != 4 or frames.shape[3] != 3 or frames.shape[0] < 1 or frames.dtype not in (torch.uint8, torch.float32):
            raise ValueError(f"MTCNN: expected a uint8 or fp32 [N, H, W, 3] tensor, got {frames.dtype} {tuple(frames.shape)}")
        dev = next(self.parameters()).device
        if dev != frames.device:
            raise L.MintimeHipError(f"MTCNN: weights on {dev}, frames on {frames.device}")
        self.check_size(frames.shape[1], frames.shape[2])
        return self.engine().run(frames.detach())

    def detect(self, img, landmarks=False):
        """The package's `detect`: img is a PIL image, an [H, W, 3] array or tensor, a list of those of equal size, or a 4-D array /
        tensor -> (boxes, probs): per image an [n, 4] array and an [n] array ordered by area (select_largest) or in NMS order, None
        and [None] for an image without a face; object arrays for a batch, the entries themselves for a single image."""
        if landmarks:
            raise NotImplementedError("MTCNN.detect(landmarks=True): the landmark head is not on the HIP path")
        batched = isinstance(img, (list, tuple)) or ((isinstance(img, np.ndarray) or torch.is_tensor(img)) and len(img.shape) == 4)
        if isinstance(img, (list, tuple)):
            arrays = [_to_uint8_array(i) for i in img]
            if any(a.shape != arrays[0].shape for a in arrays):
                raise Exception("MTCNN batch processing only compatible with equal-dimension images.")
            frames = torch.as_tensor(np.stack(arrays))
        elif torch.is_tensor(img):
            frames = img if batched else img.unsqueeze(0)
        else:
            frames = torch.as_tensor(np.asarray(img).copy())
            frames = frames if batched else frames.unsqueeze(0)
        if frames.dtype != torch.uint8:
            frames = frames.float()
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            raise L.MintimeHipError("MTCNN (MI355X build) has no CPU path: construct it with device='cuda' or move it there")
        if frames.dim() == 4:
            self.check_size(frames.shape[1], frames.shape[2])
        det = self.detect_device(frames.to(dev).contiguous())
        host = torch.cat([det.boxes, det.probs[:, None], det.frame_index.float()[:, None]], 1).cpu().numpy()      # the one read
        det.raise_on_error()
        boxes, probs = [], []
        for n in range(frames.shape[0]):
            rows = host[host[:, 5] == n]
            if len(rows) == 0:
                boxes.append(None)
                probs.append([None])
                continue
            if self.select_largest:
                area = (rows[:, 2] - rows[:, 0]) * (rows[:, 3] - rows[:, 1])
                rows = rows[np.argsort(-area, kind="stable")]
            boxes.append(rows[:, :4])
            probs.append(rows[:, 4])
        out_b, out_p = np.empty(len(boxes), dtype=object), np.empty(len(probs), dtype=object)
        for i, (b, p) in enumerate(zip(boxes, probs)):
            out_b[i], out_p[i] = b, p
        if not batched:
            return out_b[0], out_p[0]
        return out_b, out_p
