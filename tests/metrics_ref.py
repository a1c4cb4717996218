"""numpy / pure-Python restatement of the epoch metrics (mintime_amd.metrics, csrc/metrics.hip), written from the definitions in
include/mintime_hip.h and the reference lines they stand for: check_correct (utils.py:32-57), the rounded loss sum
(train.py:370, test.py:270), f1_score and roc_curve + auc (test.py:280-283).

The reference's utils.py cannot be imported here (it needs cv2, matplotlib and pytorchvideo at import time) and sklearn is not
installed, so no fixture can be generated from either: everything below is restated, and the AUC is restated twice, by two different
routes, so that the two can be held against each other (tests/test_metrics_host.py)."""
import math

import numpy as np

NUM_CLASSES = 9                  # test.py:219


def predicted(logits):
    """1 iff logit > 0 (NaN compares false: 0).  The reference's round(fp32 sigmoid(x)) differs only for 0 < x <~ 1.2e-7."""
    with np.errstate(invalid="ignore"):
        return (np.asarray(logits, dtype=np.float32).reshape(-1) > 0).astype(np.int64)


def check_correct(logits, labels, multiclass_labels=None):
    """utils.py:32-57 for one batch: dict of tp, fp, tn, fn, correct, positive, negative, errors (positions with pred != label) and,
    with multiclass_labels, mc_errors [9] (a misclassified sample counts under its class when that is a finite integer in 0..8)."""
    pred = predicted(logits)
    y = (np.asarray(labels).reshape(-1) != 0).astype(np.int64)
    assert pred.shape == y.shape
    tp = int(np.sum((pred == 1) & (y == 1)))
    fp = int(np.sum((pred == 1) & (y == 0)))
    tn = int(np.sum((pred == 0) & (y == 0)))
    fn = int(np.sum((pred == 0) & (y == 1)))
    out = dict(tp=tp, fp=fp, tn=tn, fn=fn, correct=tp + tn, positive=tp + fp, negative=tn + fn,
               errors=[int(i) for i in np.nonzero(pred != y)[0]])
    if multiclass_labels is not None:
        table = [0] * NUM_CLASSES
        for i in out["errors"]:
            c = float(np.asarray(multiclass_labels).reshape(-1)[i])
            if not math.isnan(c) and not math.isinf(c) and c == int(c) and 0 <= int(c) < NUM_CLASSES:
                table[int(c)] += 1
        out["mc_errors"] = table
    return out


def rounded_loss(loss):
    """One step's addend of the rounded sum: rint(double(loss) * 100) / 100, halves to the even integer."""
    return float(np.rint(np.float64(np.float32(loss)) * 100.0) / 100.0)


def loss_sums(losses):
    """(sum, rounded sum) of fp32 losses, added in order in fp64 -- the kernel's order."""
    s = r = 0.0
    for l in losses:
        s += float(np.float64(np.float32(l)))
        r += rounded_loss(l)
    return s, r


def f1(tp, fp, fn):
    den = 2 * tp + fp + fn
    return 2 * tp / den if den else 0.0          # sklearn: 0.0 when there is nothing to divide by


def auc_pair_counts(scores, labels):
    """(gt, eq, n_pos, n_neg) in Python integers: pairs (positive i, negative j) with score_i > / == score_j.  NaN scores take part in
    no pair and in neither class count.  Counted through sorted negatives: the same numbers as the double loop, in n log n."""
    s = np.asarray(scores, dtype=np.float32).reshape(-1)
    y = np.asarray(labels).reshape(-1) != 0
    ok = ~np.isnan(s)
    pos, neg = np.sort(s[ok & y]), np.sort(s[ok & ~y])
    below = np.searchsorted(neg, pos, side="left")          # negatives strictly below each positive
    upto = np.searchsorted(neg, pos, side="right")          # negatives below or equal
    return int(below.sum()), int((upto - below).sum()), int(pos.size), int(neg.size)


def auc_pair_counts_loop(scores, labels):
    """The definition itself, as a double loop over Python numbers (small n only): holds auc_pair_counts to it."""
    s = [float(v) for v in np.asarray(scores, dtype=np.float32).reshape(-1)]
    y = [bool(v) for v in np.asarray(labels).reshape(-1) != 0]
    pos = [v for v, l in zip(s, y) if l and not math.isnan(v)]
    neg = [v for v, l in zip(s, y) if not l and not math.isnan(v)]
    gt = sum(1 for a in pos for b in neg if a > b)
    eq = sum(1 for a in pos for b in neg if a == b)
    return gt, eq, len(pos), len(neg)


def auc_pairs(scores, labels):
    gt, eq, n_pos, n_neg = auc_pair_counts(scores, labels)
    return (2 * gt + eq) / (2 * n_pos * n_neg) if n_pos and n_neg else float("nan")


def roc_curve(scores, labels):
    """sklearn.metrics.roc_curve without drop_intermediate: one point per distinct score, descending, after the origin."""
    s = np.asarray(scores, dtype=np.float64).reshape(-1)
    y = (np.asarray(labels).reshape(-1) != 0)
    ok = ~np.isnan(s)
    s, y = s[ok], y[ok]
    order = np.argsort(-s, kind="stable")
    s, y = s[order], y[order]
    last = np.r_[np.nonzero(np.diff(s))[0], s.size - 1] if s.size else np.zeros(0, dtype=np.int64)
    tps = np.r_[0, np.cumsum(y)[last]].astype(np.float64)
    fps = np.r_[0, np.cumsum(~y)[last]].astype(np.float64)
    return fps, tps


def auc_trapezoid(scores, labels):
    """metrics.auc(fpr, tpr) over roc_curve, fp64 (test.py:281-282)."""
    fps, tps = roc_curve(scores, labels)
    if fps[-1] == 0 or tps[-1] == 0:
        return float("nan")
    fpr, tpr = fps / fps[-1], tps / tps[-1]
    return float(np.sum(np.diff(fpr) * (tpr[1:] + tpr[:-1]) / 2.0))


class Epoch:
    """The whole accumulation, host side: what EpochMetrics.compute() must return for the same sequence of updates."""

    def __init__(self, capacity, multiclass=False):
        self.capacity, self.multiclass = capacity, multiclass
        self.scores, self.labels, self.losses = [], [], []
        self.c = dict(tp=0, fp=0, tn=0, fn=0)
        self.n = self.steps = 0
        self.mc = [0] * NUM_CLASSES
        self.overflow = False

    def update(self, logits, labels, loss=None, multiclass_labels=None):
        x = np.asarray(logits, dtype=np.float32).reshape(-1)
        y = (np.asarray(labels).reshape(-1) != 0).astype(np.uint8)
        r = check_correct(x, y, multiclass_labels)
        for k in self.c:
            self.c[k] += r[k]
        if multiclass_labels is not None:
            self.mc = [a + b for a, b in zip(self.mc, r["mc_errors"])]
        self.n += x.size
        self.steps += 1
        if loss is not None:
            self.losses.append(np.float32(loss))
        room = max(self.capacity - len(self.scores), 0)
        self.scores.extend(x[:room].tolist())
        self.labels.extend(y[:room].tolist())
        self.overflow = self.overflow or x.size > room

    def compute(self):
        c = self.c
        s, r = loss_sums(self.losses)
        out = dict(n=self.n, steps=self.steps, correct=c["tp"] + c["tn"], positive=c["tp"] + c["fp"], negative=c["tn"] + c["fn"],
                   tp=c["tp"], fp=c["fp"], tn=c["tn"], fn=c["fn"], loss_sum=s, loss_sum_rounded=r, f1=f1(c["tp"], c["fp"], c["fn"]),
                   multiclass_errors=list(self.mc) if self.multiclass else None, overflow=self.overflow)
        if self.overflow:
            out.update(auc=None, error_indices=None)
        else:
            sc, lb = np.asarray(self.scores, dtype=np.float32), np.asarray(self.labels, dtype=np.uint8)
            out.update(auc=auc_pairs(sc, lb), auc_counts=auc_pair_counts(sc, lb), error_indices=check_correct(sc, lb)["errors"])
        return out
