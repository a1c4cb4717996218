"""Host side of the epoch metrics: the restatement the GPU tests compare against (tests/metrics_ref.py) is itself held to
hand-computed cases and its two AUC routes to each other; the rounded-loss rule is held to Python's round(); the two entry points
are declared and bound.  No device is touched."""
import math
import re

import numpy as np
import pytest

import mintime_amd
from mintime_amd import lib as L
from tests import metrics_ref as R
from tests.util import declared_params, header_text


def _tie_heavy(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(-8, 9, n) / 4.0).astype(np.float32), (rng.random(n) < 0.4).astype(np.uint8)


@pytest.mark.parametrize("n,seed", [(2, 0), (17, 1), (200, 2), (3000, 3)])
def test_the_two_auc_restatements_agree_on_tie_heavy_data(n, seed):
    """17 distinct scores among up to 3000 samples: most pairs across a class boundary are ties."""
    s, y = _tie_heavy(n, seed)
    a, b = R.auc_pairs(s, y), R.auc_trapezoid(s, y)
    if math.isnan(a):
        assert math.isnan(b)
    else:
        assert abs(a - b) <= 1e-12, (a, b)


@pytest.mark.parametrize("n,seed", [(1, 0), (5, 1), (64, 2), (300, 3)])
def test_sorted_pair_count_equals_the_double_loop(n, seed):
    s, y = _tie_heavy(n, seed)
    s[::7] = np.nan                                     # NaN scores: in no pair, in neither class count
    assert R.auc_pair_counts(s, y) == R.auc_pair_counts_loop(s, y)


def test_hand_computed_cases():
    """Five samples, scores [0.5, -1, 0.5, 2, 0], labels [1, 0, 0, 1, 0]:
    positives {0.5, 2}, negatives {-1, 0.5, 0}.  0.5 beats -1 and 0 and ties 0.5; 2 beats all three: gt = 5, eq = 1 of 6 pairs,
    AUC = (2*5 + 1) / (2*6) = 11/12.  As a curve: (0,0) (0,1/2) (1/3,1) (2/3,1) (1,1), area 1/3 * 3/4 + 2/3 = 11/12.
    Predictions (x > 0) are [1, 0, 1, 1, 0]: tp 2, fp 1, tn 2, fn 0, F1 = 4 / 5, the one error at position 2."""
    s, y = [0.5, -1.0, 0.5, 2.0, 0.0], [1, 0, 0, 1, 0]
    assert R.auc_pair_counts(s, y) == (5, 1, 2, 3)
    assert R.auc_pairs(s, y) == 11 / 12 and abs(R.auc_trapezoid(s, y) - 11 / 12) <= 1e-15
    c = R.check_correct(s, y)
    assert (c["tp"], c["fp"], c["tn"], c["fn"], c["correct"], c["positive"], c["negative"]) == (2, 1, 2, 0, 4, 3, 2)
    assert c["errors"] == [2] and R.f1(c["tp"], c["fp"], c["fn"]) == 0.8
    # perfect, inverse and uninformative rankings
    assert R.auc_pairs([1, 2, 3, 4], [0, 0, 1, 1]) == 1.0 == R.auc_trapezoid([1, 2, 3, 4], [0, 0, 1, 1])
    assert R.auc_pairs([1, 2, 3, 4], [1, 1, 0, 0]) == 0.0 == R.auc_trapezoid([1, 2, 3, 4], [1, 1, 0, 0])
    assert R.auc_pairs([7, 7, 7, 7, 7], [1, 0, 0, 1, 0]) == 0.5 == R.auc_trapezoid([7, 7, 7, 7, 7], [1, 0, 0, 1, 0])
    # one class only: no pair exists
    assert math.isnan(R.auc_pairs([1, 2, 3], [1, 1, 1])) and math.isnan(R.auc_trapezoid([1, 2, 3], [1, 1, 1]))
    assert math.isnan(R.auc_pairs([1, 2, 3], [0, 0, 0])) and math.isnan(R.auc_trapezoid([1, 2, 3], [0, 0, 0]))
    # nothing predicted positive and nothing positive: F1's denominator is 0
    c = R.check_correct([-1.0, -2.0], [0, 0])
    assert R.f1(c["tp"], c["fp"], c["fn"]) == 0.0


def test_prediction_rule_edges():
    """x = 0 and NaN are class 0; the smallest positive float is class 1 (the documented window against round(sigmoid(x)))."""
    x = np.array([0.0, -0.0, np.nan, np.float32(1e-45), 5e-8, 1.1e-7, -1e-30], dtype=np.float32)
    assert R.predicted(x).tolist() == [0, 0, 0, 1, 1, 1, 0]


def test_multiclass_table_skips_nan_and_out_of_range():
    x = np.array([1.0] * 8, dtype=np.float32)                        # all predicted 1
    y = np.zeros(8)                                                   # all wrong
    mc = np.array([np.nan, 0, 8, 9, -1, 3, 3, 2.5], dtype=np.float32)
    assert R.check_correct(x, y, mc)["mc_errors"] == [1, 0, 0, 2, 0, 0, 0, 0, 1]
    assert R.check_correct(x, np.ones(8), mc)["mc_errors"] == [0] * 9        # all right: nothing counted


def test_rint_rule_is_pythons_round_to_two_places():
    """total_loss += round(loss.item(), 2) (train.py:370): rint(double(loss) * 100) / 100 gives the same double on every one of
    10^5 seeded fp32 losses in [0, 3)."""
    losses = (np.random.default_rng(0).random(100000) * 3.0).astype(np.float32)
    bad = sum(1 for l in losses if R.rounded_loss(l) != round(float(l), 2))
    assert bad == 0
    s, r = R.loss_sums(losses[:100])
    want_s = want_r = 0.0
    for l in losses[:100]:
        want_s += float(l)
        want_r += round(float(l), 2)
    assert (s, r) == (want_s, want_r)


def test_epoch_restatement_overflow_and_store_order():
    e = R.Epoch(capacity=5)
    e.update([1.0, -1.0, 2.0], [1, 1, 0], loss=0.125)
    assert e.compute()["error_indices"] == [1, 2] and not e.compute()["overflow"]
    e.update([3.0, 4.0, 5.0], [1, 1, 1], loss=0.375)
    r = e.compute()
    assert r["overflow"] and r["auc"] is None and r["error_indices"] is None
    assert (r["n"], r["steps"], r["tp"], r["fp"], r["fn"], r["tn"]) == (6, 2, 4, 1, 1, 0)
    assert e.scores == [1.0, -1.0, 2.0, 3.0, 4.0] and r["loss_sum"] == 0.5 and r["loss_sum_rounded"] == 0.12 + 0.38


@pytest.mark.parametrize("name,count", [("mt_metrics_update", 12), ("mt_metrics_auc", 6)])
def test_entry_point_is_declared_and_bound(name, count):
    params = declared_params(name)
    assert params[-1] == "void* stream"                          # a launching entry point: csrc/gen_plan.py gives it a recording thunk
    assert name in L.PROTOTYPES and len(L.PROTOTYPES[name]) == len(params) == count
    import ctypes
    handle = ctypes.CDLL(L.LIB_PATH)
    assert hasattr(handle, name) and hasattr(handle, "mti_" + name[3:])


def test_package_surface_and_documented_windows():
    assert mintime_amd.EpochMetrics is mintime_amd.metrics.EpochMetrics
    m = mintime_amd.metrics
    assert (m.AUC_BLOCK, m.AUC_TILE, m.AUC_MAX_N, m.NUM_CLASSES) == (256, 1024, 1 << 24, R.NUM_CLASSES)
    hdr = header_text()
    decl = hdr[hdr.index("Epoch metrics"):hdr.index("int mt_metrics_auc")]
    assert "1.2e-7" in decl and "16.6" in decl                   # the two deviation windows are stated where the ABI is
    assert re.search(r"#define\s+MT_VERSION\s+(\d+)", hdr).group(1) == str(L.ABI_VERSION)


def test_epoch_metrics_has_no_cpu_path():
    with pytest.raises(ValueError, match="no CPU path"):
        mintime_amd.EpochMetrics(capacity=4, device="cpu")
