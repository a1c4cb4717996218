"""FaceNet InceptionResnetV1: the face embedder in front of the identity clustering (identities.py), inference only, on the HIP path
(facenet_engine.py, csrc/facenet.hip).

The reference takes `facenet_pytorch.InceptionResnetV1(pretrained='vggface2').eval()` (predict.py:150-158,
preprocessing/cluster_faces.py:84-92).  This module rebuilds that network from its published structure, with the package's module
names, so a facenet_pytorch state dict loads (`weights_path`, or `load_state_dict`; a `module.` prefix is stripped):

    from mintime_amd import InceptionResnetV1, fixed_image_standardization
    embedder = InceptionResnetV1(pretrained='vggface2', weights_path='20180402-114759-vggface2.pt', device='cuda').eval()
    embeddings = embedder(faces)                  # faces [T, 3, H, W] fp32, standardised (the reference's call)
    embeddings = embedder.embed_crops(crops)      # crops [T, H, W, 3] uint8 or raw fp32: the standardisation rides in the ingest

UNCHECKED against facenet_pytorch: the package is not available where this was written, so the structure and the key names below
(714 state-dict entries without `logits`, 23 482 624 parameters, 132 Conv2d; tests/golden/facenet_inception_resnet_v1_manifest.json)
are restated by hand from its published source and have not been compared with the package or a real checkpoint.

Not covered: `classify=True` (the `logits` layer is held for the state dict and never launched), training / fine-tuning (no backward),
downloading weights.  (The detector is mtcnn.py, the crops face_crops.py.)  The returned [T, 512] tensor is a buffer of the module, overwritten by
the next call with the same T; H and W of at least 75.  There is no CPU path."""
import torch
from torch import nn

from . import facenet_engine as E
from . import lib as L

PRETRAINED_CLASSES = {"vggface2": 8631, "casia-webface": 10575}


def fixed_image_standardization(image_tensor):
    return (image_tensor - 127.5) / 128.0


def _never(self, *a, **k):
    raise L.MintimeHipError("InceptionResnetV1 submodules only hold weights: call the network (its HIP engine runs the layers)")


class BasicConv2d(nn.Module):
    def __init__(self, in_planes, out_planes, kernel_size, stride=1, padding=0):
        super().__init__()
        self.conv = nn.Conv2d(in_planes, out_planes, kernel_size=kernel_size, stride=stride, padding=padding, bias=False)
        self.bn = nn.BatchNorm2d(out_planes, eps=0.001, momentum=0.1, affine=True)

    forward = _never


class Block35(nn.Module):
    def __init__(self, scale=1.0):
        super().__init__()
        self.scale = scale
        self.noReLU = False
        self.branch0 = BasicConv2d(256, 32, 1)
        self.branch1 = nn.Sequential(BasicConv2d(256, 32, 1), BasicConv2d(32, 32, 3, padding=1))
        self.branch2 = nn.Sequential(BasicConv2d(256, 32, 1), BasicConv2d(32, 32, 3, padding=1), BasicConv2d(32, 32, 3, padding=1))
        self.conv2d = nn.Conv2d(96, 256, kernel_size=1)

    forward = _never


class Block17(nn.Module):
    def __init__(self, scale=1.0):
        super().__init__()
        self.scale = scale
        self.noReLU = False
        self.branch0 = BasicConv2d(896, 128, 1)
        self.branch1 = nn.Sequential(BasicConv2d(896, 128, 1), BasicConv2d(128, 128, (1, 7), padding=(0, 3)),
                                     BasicConv2d(128, 128, (7, 1), padding=(3, 0)))
        self.conv2d = nn.Conv2d(256, 896, kernel_size=1)

    forward = _never


class Block8(nn.Module):
    def __init__(self, scale=1.0, noReLU=False):
        super().__init__()
        self.scale = scale
        self.noReLU = noReLU
        self.branch0 = BasicConv2d(1792, 192, 1)
        self.branch1 = nn.Sequential(BasicConv2d(1792, 192, 1), BasicConv2d(192, 192, (1, 3), padding=(0, 1)),
                                     BasicConv2d(192, 192, (3, 1), padding=(1, 0)))
        self.conv2d = nn.Conv2d(384, 1792, kernel_size=1)

    forward = _never


class Mixed_6a(nn.Module):
    def __init__(self):
        super().__init__()
        self.branch0 = BasicConv2d(256, 384, 3, stride=2)
        self.branch1 = nn.Sequential(BasicConv2d(256, 192, 1), BasicConv2d(192, 192, 3, padding=1), BasicConv2d(192, 256, 3, stride=2))
        self.branch2 = nn.MaxPool2d(3, stride=2)

    forward = _never


class Mixed_7a(nn.Module):
    def __init__(self):
        super().__init__()
        self.branch0 = nn.Sequential(BasicConv2d(896, 256, 1), BasicConv2d(256, 384, 3, stride=2))
        self.branch1 = nn.Sequential(BasicConv2d(896, 256, 1), BasicConv2d(256, 256, 3, stride=2))
        self.branch2 = nn.Sequential(BasicConv2d(896, 256, 1), BasicConv2d(256, 256, 3, padding=1), BasicConv2d(256, 256, 3, stride=2))
        self.branch3 = nn.MaxPool2d(3, stride=2)

    forward = _never


class InceptionResnetV1(nn.Module):
    """facenet_pytorch's constructor signature plus `weights_path` (a local facenet_pytorch state dict; nothing is downloaded)."""

    def __init__(self, pretrained=None, classify=False, num_classes=None, dropout_prob=0.6, device=None, weights_path=None):
        super().__init__()
        if classify:
            raise NotImplementedError("InceptionResnetV1(classify=True): the logits layer is not on the HIP path (embeddings only)")
        if pretrained is not None:
            if pretrained not in PRETRAINED_CLASSES:
                raise ValueError(f"pretrained={pretrained!r} is not one of {sorted(PRETRAINED_CLASSES)}")
            if weights_path is None:
                raise RuntimeError(f"InceptionResnetV1(pretrained={pretrained!r}) downloads a checkpoint, which needs network access; pass "
                                   "weights_path= to a local facenet_pytorch state dict")
            num_classes = PRETRAINED_CLASSES[pretrained]
        self.pretrained, self.classify, self.num_classes = pretrained, False, num_classes
        self.conv2d_1a = BasicConv2d(3, 32, 3, stride=2)
        self.conv2d_2a = BasicConv2d(32, 32, 3)
        self.conv2d_2b = BasicConv2d(32, 64, 3, padding=1)
        self.maxpool_3a = nn.MaxPool2d(3, stride=2)
        self.conv2d_3b = BasicConv2d(64, 80, 1)
        self.conv2d_4a = BasicConv2d(80, 192, 3)
        self.conv2d_4b = BasicConv2d(192, 256, 3, stride=2)
        self.repeat_1 = nn.Sequential(*[Block35(scale=0.17) for _ in range(5)])
        self.mixed_6a = Mixed_6a()
        self.repeat_2 = nn.Sequential(*[Block17(scale=0.10) for _ in range(10)])
        self.mixed_7a = Mixed_7a()
        self.repeat_3 = nn.Sequential(*[Block8(scale=0.20) for _ in range(5)])
        self.block8 = Block8(noReLU=True)
        self.avgpool_1a = nn.AdaptiveAvgPool2d(1)
        self.dropout = nn.Dropout(dropout_prob)
        self.last_linear = nn.Linear(1792, 512, bias=False)
        self.last_bn = nn.BatchNorm1d(512, eps=0.001, momentum=0.1, affine=True)
        if num_classes is not None:
            self.logits = nn.Linear(512, num_classes)          # held for the checkpoint's keys; never launched
        if weights_path is not None:
            self.load_state_dict(torch.load(weights_path, map_location="cpu"))
        self.device = torch.device("cpu")
        if device is not None:
            self.device = torch.device(device)
            self.to(self.device)
        self._engine = None

    def load_state_dict(self, state_dict, strict=True, **kw):
        sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in state_dict.items()}
        return super().load_state_dict(sd, strict=strict, **kw)

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

    def _check(self, t, what):
        if self.training:
            raise NotImplementedError("InceptionResnetV1 (MI355X build) is inference only: call .eval() first (there is no backward)")
        if not torch.is_tensor(t) or not t.is_cuda:
            raise L.MintimeHipError(f"InceptionResnetV1 (MI355X build) needs device tensors; {what} is on the CPU and there is no CPU path")
        if next(self.parameters()).device != t.device:
            raise L.MintimeHipError(f"InceptionResnetV1: weights on {next(self.parameters()).device}, {what} on {t.device}")

    def forward(self, x):
        """x: fp32 [T, 3, H, W], already standardised; contiguous or the view faces.permute(0, 3, 1, 2) of a channels-last array
        (read in place) -> [T, 512] fp32, unit rows, no grad_fn."""
        self._check(x, "x")
        if x.dim() != 4 or x.shape[1] != 3 or x.dtype != torch.float32:
            raise ValueError(f"InceptionResnetV1: expected an fp32 [T, 3, H, W] tensor, got {x.dtype} {tuple(x.shape)}")
        T, _, H, W = x.shape
        E.check_side(H, W)
        x = x.detach()
        if T == 0:
            return x.new_empty(0, 512)
        s = x.stride()
        return self.engine().run(x, False, (s[0], s[2], s[3], s[1]), T, H, W, False)

    def embed_crops(self, crops):
        """crops: [T, H, W, 3] uint8 or fp32 with raw 0..255 values, on the device -> [T, 512] fp32:
        forward(fixed_image_standardization(crops.permute(0, 3, 1, 2).float())) with the standardisation done by the ingest."""
        self._check(crops, "crops")
        if crops.dim() != 4 or crops.shape[3] != 3 or crops.dtype not in (torch.uint8, torch.float32):
            raise ValueError(f"embed_crops: expected a uint8 or fp32 [T, H, W, 3] tensor, got {crops.dtype} {tuple(crops.shape)}")
        T, H, W, _ = crops.shape
        E.check_side(H, W)
        crops = crops.detach()
        if T == 0:
            return torch.empty(0, 512, dtype=torch.float32, device=crops.device)
        return self.engine().run(crops, crops.dtype == torch.uint8, tuple(crops.stride()), T, H, W, True)
