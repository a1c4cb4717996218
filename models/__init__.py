"""Drop-in boundary: the reference's `models` package paths, backed by the MI355X-native implementation.

    from models.efficientnet.efficientnet_pytorch import EfficientNet      (reference train.py:27)
    from models.size_invariant_timesformer import SizeInvariantTimeSformer (reference train.py:28)
    from models.baseline import Baseline                                   (reference train.py:32)
    from models.xception import xception                                   (reference train.py:33)
    from models.slowfast import slowfast_r50                               (reference train.py:145 via torch.hub; hubconf.py)
"""
