"""Drop-in for the reference's metrics.py (accuracy, micro/macro F1)."""


def accuracy(output, labels):
    """Fraction of argmax predictions equal to labels, as a 0-d double tensor
    (reference metrics.py:3-7)."""
    preds = output.max(1)[1].type_as(labels)
    return preds.eq(labels).double().sum() / len(labels)


def f1(output, labels):
    """(micro, macro) F1 via sklearn on host copies (reference metrics.py:9-15)."""
    from sklearn.metrics import f1_score
    preds = output.max(1)[1].cpu().detach().numpy()
    labels = labels.cpu().detach().numpy()
    return f1_score(labels, preds, average="micro"), f1_score(labels, preds, average="macro")


def f1_from_confusion(cm):
    """(micro, macro) F1 of a confusion matrix (row = label, column =
    prediction), with sklearn.metrics.f1_score's formulas: per class
    f_c = 2 tp_c / (true_c + pred_c), 0 where the denominator is 0; macro is
    the mean over the classes present in labels or predictions (sklearn's
    unique_labels); micro takes the summed counts.  Pure numpy."""
    import numpy as np
    cm = np.asarray(cm, dtype=np.int64)
    tp = np.diag(cm)
    denom = cm.sum(1) + cm.sum(0)  # true_c + pred_c = 2 tp + fp + fn
    present = denom > 0
    if not present.any():
        return 0.0, 0.0
    f = np.zeros(len(tp), dtype=np.float64)
    f[present] = 2.0 * tp[present] / denom[present]
    micro = 2.0 * tp.sum() / denom.sum()
    return float(micro), float(f[present].mean())


class Evaluation:
    """What SGC.evaluate leaves on the device: `.confusion` (int64 [C, C], row =
    label, column = prediction), `.count` and `.correct` (int64 0-d: the rows
    counted and the rows predicted right) and `.loss` (float32 0-d, the mean
    cross-entropy).  `n` is len(labels)."""

    def __init__(self, confusion, count, correct, loss, n):
        self.confusion, self.count, self.correct, self.loss, self.n = (confusion, count, correct,
                                                                       loss, n)

    def accuracy(self):
        """accuracy(model(x), labels): a 0-d double tensor, correct / len(labels)."""
        return self.correct.double() / self.n

    def f1(self):
        """f1(model(x), labels): (micro, macro) floats from one read-back of the matrix."""
        return f1_from_confusion(self.confusion.cpu().numpy())
