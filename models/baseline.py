"""Drop-in for reference models/baseline.py: `Baseline(config)` (train.py:137-138, test.py:115-116, `--model 0`), HIP-backed."""
import mintime_amd as _impl

Baseline = _impl.Baseline

__all__ = ["Baseline"]
