"""SlowFast R50 of the reference's `--model 2` (train.py:143-147, test.py:121-125), HIP-backed: pytorchvideo's `slowfast_r50`
structure and state-dict names.  `torch.hub.load(<repository dir>, 'slowfast_r50', source='local')` reaches it through hubconf.py."""
import mintime_amd as _impl

slowfast_r50 = _impl.slowfast_r50
SlowFast = _impl.SlowFast

__all__ = ["slowfast_r50", "SlowFast"]
