"""torch.hub entry points of this repository: the reference's
    torch.hub.load('facebookresearch/pytorchvideo', 'slowfast_r50', pretrained=True)          (train.py:145, test.py:123)
becomes
    torch.hub.load('<path of this repository>', 'slowfast_r50', source='local')
(pretrained=True needs weights_path=<local checkpoint>: there is no download)."""
import os
import sys

dependencies = ["torch"]

_ROOT = os.path.dirname(os.path.abspath(__file__))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from models.slowfast import slowfast_r50  # noqa: E402,F401
