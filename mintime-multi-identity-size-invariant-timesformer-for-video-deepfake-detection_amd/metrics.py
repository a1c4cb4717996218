"""Epoch metrics on the device (next-row f5): what the reference's step bodies do on the host after `y_pred.cpu()` every step --
`check_correct` (utils.py:32-57 at train.py:367-374, :434-441, test.py:267-277) and `total_loss += round(loss.item(), 2)` -- and what
test.py:280-283 computes with sklearn at the end of a run (roc_curve + auc, f1_score, the per-method error table, the list of
misclassified videos).  `update` is one launch into device state and reads nothing back; `compute` is the only call that synchronises.

Two documented deviations from the reference (csrc/metrics.hip):
  * predicted class is `logit > 0`; the reference's `round(fp32 sigmoid(logit))` gives 0 instead of 1 for 0 < logit <~ 1.2e-7, where
    fp32 sigmoid returns exactly 0.5;
  * the AUC ranks the logits, the reference ranks fp32 sigmoid(logit): they differ only where distinct logits collapse to one sigmoid
    value (saturation from about |logit| > 16.6, or neighbours closer than an ulp of the sigmoid)."""
import torch

from . import lib as L

AUC_BLOCK = 256          # samples per block of the all-pairs kernel (csrc/metrics.hip)
AUC_TILE = 1024          # scores per LDS tile there
AUC_MAX_N = 1 << 24      # mt_metrics_auc refuses more
NUM_CLASSES = 9          # test.py:219

_SEEN, _TP, _FP, _TN, _FN, _STEPS, _STORED, _OVERFLOW, _SLOTS = range(9)     # counts[] of mt_metrics_update


class EpochMetrics:
    """Counters, loss sums, the multiclass error table and a fixed-capacity store of (logit, label) pairs, all in device memory.

        m = EpochMetrics(capacity=len(dataset))
        for batch in loader:  ...;  m.update(y_pred, labels, loss)          # no sync
        r = m.compute()                                                     # one sync: r["accuracy"], r["f1"], r["auc"], ...

    When more than `capacity` samples arrive the store keeps the first `capacity`, `overflow` is set, the counters still count every
    sample, and `auc` / `error_indices` are None (never computed from a truncated store).  `store_scores` [capacity] fp32 and
    `store_labels` [capacity] uint8 are plain tensors and may be replaced by views of the caller's own memory before the first update.
    Not covered: merging across data-parallel ranks (the counters could be summed; the AUC needs the gathered scores)."""

    def __init__(self, capacity=65536, device="cuda", multiclass=False):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise ValueError("EpochMetrics lives on the device (there is no CPU path)")
        if capacity < 0:
            raise ValueError("capacity must be non-negative")
        self.capacity = int(capacity)
        self.multiclass = bool(multiclass)
        self.device = dev
        self._ints = L.zeros(_SLOTS + NUM_CLASSES, torch.int64, dev)          # counts [8] then mc_errors [9]
        self._loss = L.zeros(2, torch.float64, dev)
        self.store_scores = torch.empty(max(self.capacity, 1), dtype=torch.float32, device=dev)[:self.capacity]
        self.store_labels = torch.empty(max(self.capacity, 1), dtype=torch.uint8, device=dev)[:self.capacity]

    def reset(self):
        L.zero_(self._ints)
        L.zero_(self._loss)

    @torch.no_grad()
    def update(self, logits, labels, loss=None, multiclass_labels=None):
        """Accumulate one step.  logits [B] or [B,1]; labels any numeric dtype, 0 / 1; loss: the step's scalar loss tensor (on the
        device); multiclass_labels [B] float, NaN where the video has no class (needs multiclass=True).  One launch, nothing read back."""
        for name, t in (("logits", logits), ("labels", labels), ("loss", loss), ("multiclass_labels", multiclass_labels)):
            if t is not None and not (torch.is_tensor(t) and t.is_cuda):
                raise ValueError(f"EpochMetrics.update: {name} must be a tensor on the device (there is no CPU path)")
        if multiclass_labels is not None and not self.multiclass:
            raise ValueError("EpochMetrics.update: multiclass_labels given, but the object was built with multiclass=False")
        n = logits.numel()
        if n == 0 or labels.numel() != n or (multiclass_labels is not None and multiclass_labels.numel() != n):
            raise ValueError("EpochMetrics.update: logits, labels and multiclass_labels must hold the same, non-zero number of elements")
        if loss is not None and loss.numel() != 1:
            raise ValueError("EpochMetrics.update: loss must be a scalar")
        x = logits.detach().reshape(-1).float().contiguous()
        y = labels.detach().reshape(-1).to(torch.float32).contiguous()
        lo = None if loss is None else loss.detach().reshape(1).float()
        mc = None if multiclass_labels is None else multiclass_labels.detach().reshape(-1).to(torch.float32).contiguous()
        if self.store_scores.numel() != self.capacity or self.store_labels.numel() != self.capacity:
            raise ValueError("EpochMetrics.update: the sample store does not hold `capacity` elements")
        L.mt.metrics_update(x, y, lo, mc, self._ints, self._loss, self._ints[_SLOTS:], self.store_scores, self.store_labels,
                            self.capacity, n)

    def auc_counts(self, n=None):
        """(gt, eq, n_pos, n_neg) of the first n stored samples (default: all of them), as Python ints: the number of (positive,
        negative) pairs whose scores compare > / ==, and the class counts without NaN scores.  AUC = (2 gt + eq) / (2 n_pos n_neg).
        Synchronises."""
        if n is None:
            n = int(self._ints[_STORED])
        blocks = (n + AUC_BLOCK - 1) // AUC_BLOCK
        partials = torch.empty(max(4 * blocks, 1), dtype=torch.int64, device=self.device)
        out = torch.empty(4, dtype=torch.int64, device=self.device)
        L.mt.metrics_auc(self.store_scores, self.store_labels, n, partials, out)
        return tuple(out.cpu().tolist())

    def compute(self):
        """Everything the reference prints at the end of an epoch / test run, as Python numbers.  Synchronises with the device."""
        ints = self._ints.cpu().tolist()
        loss_sum, loss_rounded = self._loss.cpu().tolist()
        tp, fp, tn, fn = ints[_TP], ints[_FP], ints[_TN], ints[_FN]
        n, steps, stored, overflow = ints[_SEEN], ints[_STEPS], ints[_STORED], bool(ints[_OVERFLOW])
        auc, errors = None, None
        if not overflow:
            gt, eq, n_pos, n_neg = self.auc_counts(stored)
            auc = (2 * gt + eq) / (2 * n_pos * n_neg) if n_pos and n_neg else float("nan")
            wrong = (self.store_scores[:stored] > 0) != (self.store_labels[:stored] != 0)
            errors = torch.nonzero(wrong).reshape(-1).cpu().tolist()
        return {
            "n": n, "steps": steps, "correct": tp + tn, "positive": tp + fp, "negative": tn + fn,
            "tp": tp, "fp": fp, "tn": tn, "fn": fn,
            "accuracy": (tp + tn) / n if n else float("nan"),
            "loss_sum": loss_sum, "loss_sum_rounded": loss_rounded,
            "loss_mean_rounded": loss_rounded / steps if steps else float("nan"),       # the reference's total_loss /= counter
            "f1": 2 * tp / (2 * tp + fp + fn) if (2 * tp + fp + fn) else 0.0,           # sklearn's value for 0 / 0
            "auc": auc, "error_indices": errors,
            "multiclass_errors": ints[_SLOTS:_SLOTS + NUM_CLASSES] if self.multiclass else None,
            "overflow": overflow,
        }
