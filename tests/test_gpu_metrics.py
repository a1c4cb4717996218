"""Epoch metrics on the device (mintime_amd.EpochMetrics; csrc/metrics.hip: mt_metrics_update, mt_metrics_auc) against the numpy
restatement tests/metrics_ref.py.  Every comparison is between integers or fp64 sums added in the same order: the integer fields
and the rounded loss sum must be equal, the plain loss sum equal to 1e-12 relative (the restatement adds the same doubles in the
same order, so equality is what is expected there too).

Logits come from the grid k / 64, k in [-256, 256]: fp32 sigmoid is strictly increasing on it (smallest gap 2.8e-4), so ranking by
logit and ranking by sigmoid coincide, exact ties are frequent and x = 0 occurs.  Labels are seeded Bernoulli(0.4)."""
import math

import numpy as np
import pytest
import torch

import mintime_amd
from mintime_amd import EpochMetrics, harness, metrics
from mintime_amd import lib as L
from tests import metrics_ref as R

pytestmark = pytest.mark.gpu

BATCHES = (1, 1, 7, 64, 33, 256, 257, 381)              # 1000 samples: below, at and above the update kernel's 256 threads
INT_FIELDS = ("n", "steps", "correct", "positive", "negative", "tp", "fp", "tn", "fn")
TILE, BLOCK = metrics.AUC_TILE, metrics.AUC_BLOCK


def _data(n, seed):
    rng = np.random.default_rng(seed)
    x = (rng.integers(-256, 257, n) / 64.0).astype(np.float32)
    y = (rng.random(n) < 0.4).astype(np.uint8)
    return x, y


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def _one_update(x, y, capacity=None):
    m = EpochMetrics(capacity=len(x) if capacity is None else capacity)
    m.update(_dev(x), _dev(y))
    return m


@pytest.fixture(scope="module")
def epoch():
    """Eight updates of mixed shapes and label dtypes with a loss and class labels each: (EpochMetrics result, restatement result)."""
    rng = np.random.default_rng(7)
    classes = np.array([np.nan, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, -1], dtype=np.float32)
    m, ref = EpochMetrics(capacity=1000, multiclass=True), R.Epoch(1000, multiclass=True)
    for step, b in enumerate(BATCHES):
        x, y = _data(b, 100 + step)
        if step == 3:
            x[:8] = 0.0                                          # x = 0 is class 0
        mc = classes[rng.integers(0, len(classes), b)]
        loss = np.float32(rng.random() * 3.0)
        xd = _dev(x).reshape(b, 1) if step % 2 else _dev(x)                             # [B, 1] and [B]
        yd = _dev(y, torch.int64) if step % 3 == 0 else _dev(y, torch.float32)
        if step % 2 == 0:
            yd = yd.reshape(b, 1)                                                        # labels.unsqueeze(1) (train.py:336) against [B] logits too
        m.update(xd, yd, _dev(np.array(loss)), _dev(mc))
        ref.update(x, y, loss, mc)
    return m, m.compute(), ref.compute(), ref


def test_counters_equal_the_restatement(epoch):
    _, got, want, _ = epoch
    for k in INT_FIELDS:
        assert type(got[k]) is int and got[k] == want[k], (k, got[k], want[k])
    assert got["n"] == 1000 and got["steps"] == 8 and got["correct"] + got["fp"] + got["fn"] == 1000
    assert got["accuracy"] == want["correct"] / 1000 and got["f1"] == want["f1"]
    assert got["overflow"] is False


def test_loss_sums(epoch):
    _, got, want, _ = epoch
    assert abs(got["loss_sum"] - want["loss_sum"]) <= 1e-12 * abs(want["loss_sum"]), (got["loss_sum"], want["loss_sum"])
    assert got["loss_sum_rounded"] == want["loss_sum_rounded"]
    assert got["loss_mean_rounded"] == want["loss_sum_rounded"] / 8


def test_multiclass_table(epoch):
    """Classes drawn from {NaN, 0..8, 9, -1}: NaN, 9 and -1 are in no cell."""
    _, got, want, _ = epoch
    assert got["multiclass_errors"] == want["multiclass_errors"] and len(got["multiclass_errors"]) == 9
    assert all(type(v) is int for v in got["multiclass_errors"])
    assert 0 < sum(got["multiclass_errors"]) < got["fp"] + got["fn"]                # some errors had no countable class


def test_error_indices_and_auc_of_the_epoch(epoch):
    m, got, want, ref = epoch
    assert got["error_indices"] == want["error_indices"] and len(got["error_indices"]) == got["fp"] + got["fn"]
    assert m.auc_counts() == want["auc_counts"]
    assert got["auc"] == want["auc"]
    assert abs(got["auc"] - R.auc_trapezoid(np.asarray(ref.scores), np.asarray(ref.labels))) <= 1e-12
    assert torch.equal(m.store_scores.cpu(), torch.tensor(ref.scores)) and m.store_labels.cpu().tolist() == ref.labels


def test_multiclass_is_none_without_the_table():
    x, y = _data(5, 1)
    assert _one_update(x, y).compute()["multiclass_errors"] is None


@pytest.mark.parametrize("n", [1, 2, BLOCK - 1, BLOCK, BLOCK + 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 17, 3000])
def test_auc_counts_are_exact(n):
    """The integer numerator parts and both class counts, at one and two samples, around the block (256) and the LDS tile (1024),
    with a ragged last tile, and over several blocks and tiles."""
    x, y = _data(n, n)
    m = _one_update(x, y)
    want = R.auc_pair_counts(x, y)
    assert m.auc_counts() == want
    got = m.compute()["auc"]
    if want[2] and want[3]:
        assert got == (2 * want[0] + want[1]) / (2 * want[2] * want[3])
    else:
        assert math.isnan(got)


def test_auc_special_cases():
    n = 700
    y = (np.arange(n) % 3 == 0).astype(np.uint8)
    up = np.where(y == 1, 1.0, -1.0).astype(np.float32) + (np.arange(n) % 5).astype(np.float32) / 64.0
    assert _one_update(up, y).compute()["auc"] == 1.0                            # perfect separation
    assert _one_update(-up, y).compute()["auc"] == 0.0                           # inverse
    assert _one_update(np.full(n, 0.25, np.float32), y).compute()["auc"] == 0.5  # all scores equal: every pair a tie
    m = _one_update(up, np.ones(n, np.uint8))
    assert math.isnan(m.compute()["auc"]) and m.auc_counts() == (0, 0, n, 0)     # only positives


def test_nan_logits_are_predicted_zero_and_take_part_in_no_pair():
    n = 600
    x, y = _data(n, 5)
    x[::9] = np.nan
    m = _one_update(x, y)
    got, want = m.compute(), R.check_correct(x, y)
    for k in ("tp", "fp", "tn", "fn"):
        assert got[k] == want[k]
    nan_pos, nan_neg = int(np.sum(np.isnan(x) & (y == 1))), int(np.sum(np.isnan(x) & (y == 0)))
    assert nan_pos and nan_neg
    assert got["fn"] >= nan_pos and got["tn"] >= nan_neg                          # counted, as class 0
    counts = m.auc_counts()
    assert counts == R.auc_pair_counts(x, y) == R.auc_pair_counts(x[~np.isnan(x)], y[~np.isnan(x)])
    assert counts[2] == int(y.sum()) - nan_pos and counts[3] == n - int(y.sum()) - nan_neg
    assert got["error_indices"] == want["errors"]


def test_overflow_keeps_counting_and_writes_nothing_past_the_store():
    """capacity 100, 130 samples in three updates (the second straddles the end): counters exact, overflow set, auc and
    error_indices withheld, and the 28 elements after the store inside a poisoned tensor untouched."""
    x, y = _data(130, 11)
    big_x = torch.full((128,), -7.5, dtype=torch.float32, device="cuda")
    big_y = torch.full((128,), 0xAB, dtype=torch.uint8, device="cuda")
    m = EpochMetrics(capacity=100)
    m.store_scores, m.store_labels = big_x[:100], big_y[:100]
    ref = R.Epoch(100)
    for lo, hi in ((0, 60), (60, 110), (110, 130)):
        m.update(_dev(x[lo:hi]), _dev(y[lo:hi]))
        ref.update(x[lo:hi], y[lo:hi])
    got, want = m.compute(), ref.compute()
    for k in INT_FIELDS:
        assert got[k] == want[k], k
    assert got["n"] == 130 and got["overflow"] is True and got["auc"] is None and got["error_indices"] is None
    assert torch.equal(big_x[:100].cpu(), torch.from_numpy(x[:100])) and torch.equal(big_y[:100].cpu(), torch.from_numpy(y[:100]))
    assert bool((big_x[100:] == -7.5).all()) and bool((big_y[100:] == 0xAB).all())
    m.reset()                                                                     # a reset clears the flag and the position
    m.update(_dev(x[:10]), _dev(y[:10]))
    r = m.compute()
    assert r["overflow"] is False and r["n"] == 10 and r["error_indices"] == R.check_correct(x[:10], y[:10])["errors"]


def test_reset_zeroes_everything():
    x, y = _data(50, 3)
    m = EpochMetrics(capacity=64, multiclass=True)
    m.update(_dev(x), _dev(y), _dev(np.array(np.float32(0.7))), _dev(np.zeros(50, np.float32)))
    assert m.compute()["n"] == 50
    m.reset()
    r = m.compute()
    for k in INT_FIELDS:
        assert r[k] == 0, k
    assert r["loss_sum"] == 0.0 and r["loss_sum_rounded"] == 0.0 and r["multiclass_errors"] == [0] * 9
    assert r["f1"] == 0.0 and math.isnan(r["auc"]) and r["error_indices"] == [] and r["overflow"] is False
    assert m.auc_counts() == (0, 0, 0, 0)                                         # n = 0: zeros, nothing launched


def test_update_replays_from_a_captured_graph():
    """One update of a static 16-sample batch captured on a single stream and replayed three times: the append position comes from
    the device state, so every replay lands behind the previous one."""
    x, y = _data(16, 21)
    xd, yd, ld = _dev(x), _dev(y, torch.float32), _dev(np.array(np.float32(0.625)))
    m = EpochMetrics(capacity=64)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.update(xd, yd, ld)                                                      # loads the kernel outside the capture
    torch.cuda.current_stream().wait_stream(side)
    single = m.compute()
    m.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        m.update(xd, yd, ld)
    for _ in range(3):
        graph.replay()
    got = m.compute()
    for k in INT_FIELDS:
        assert got[k] == 3 * single[k], k
    assert got["n"] == 48 and got["steps"] == 3
    assert got["loss_sum"] == 3 * 0.625 and got["loss_sum_rounded"] == 0.62 + 0.62 + 0.62      # rint(62.5) = 62: halves to even
    assert torch.equal(m.store_scores[:48].cpu(), torch.from_numpy(np.tile(x, 3)))
    assert torch.equal(m.store_labels[:48].cpu(), torch.from_numpy(np.tile(y, 3)))
    assert got["error_indices"] == [i + 16 * r for r in range(3) for i in single["error_indices"]]


def test_train_step_with_metrics_changes_no_bit():
    """harness.train_step at 2 clips from the same state, with and without metrics=: same loss, same parameters, bit for bit
    (deterministic mode, so that two runs of the same step are comparable at all)."""
    prev = L.set_deterministic(True)
    try:
        def run(m):
            torch.manual_seed(5)
            cfg, ef, tsf = harness.build_models(8, seed=1, device="cuda")
            opt = harness.make_optimizer(cfg, ef, tsf)
            batch = harness.device_batch(2, 8, 2, seed=0, device="cuda")
            loss = harness.train_step(ef, tsf, opt, batch, metrics=m).detach().clone()
            torch.cuda.synchronize()
            return loss, [p.detach().clone() for p in list(ef.parameters()) + list(tsf.parameters())], batch

        m = EpochMetrics(capacity=8)
        loss_a, params_a, _ = run(None)
        loss_b, params_b, batch = run(m)
    finally:
        L.set_deterministic(prev)
    assert torch.equal(loss_a, loss_b)
    assert len(params_a) == len(params_b) and all(torch.equal(a, b) for a, b in zip(params_a, params_b))
    r = m.compute()
    assert r["n"] == 2 and r["steps"] == 1 and r["loss_sum"] == float(loss_b)
    assert r["positive"] + r["negative"] == 2 and m.store_labels[:2].cpu().tolist() == batch["labels"].reshape(-1).cpu().tolist()


def test_update_refuses_host_tensors_and_mismatched_sizes():
    m = EpochMetrics(capacity=8)
    x, y = torch.zeros(4, device="cuda"), torch.zeros(4, device="cuda")
    with pytest.raises(ValueError, match="no CPU path"):
        m.update(x.cpu(), y)
    with pytest.raises(ValueError, match="no CPU path"):
        m.update(x, y.cpu())
    with pytest.raises(ValueError, match="no CPU path"):
        m.update(x, y, torch.zeros(()))
    with pytest.raises(ValueError, match="same"):
        m.update(x, y[:3])
    with pytest.raises(ValueError, match="multiclass=False"):
        m.update(x, y, None, torch.zeros(4, device="cuda"))
    assert m.compute()["n"] == 0                                                 # nothing was accumulated by the refused calls
    assert L.get().mt_metrics_auc(None, None, (1 << 24) + 1, None, L.ptr(torch.zeros(4, dtype=torch.int64, device="cuda")),
                                  L.stream_ptr()) == -3                          # MT_ERR_UNSUPPORTED, nothing launched
