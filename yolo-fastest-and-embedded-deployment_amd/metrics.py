"""yolov5's detection metrics (its utils/metrics.py: compute_ap, ap_per_class, smooth, fitness) in numpy float64, on the true-positive flags
that `Validation.get_metrics` collects.  Host arithmetic: a few thousand rows per validation pass.  Two departures from yolov5, both
stated where they happen: the ranking sort is stable, and every class of the model has a row (yolov5 has one per class that has labels)."""
import numpy as np

_trapezoid = getattr(np, "trapezoid", None) or np.trapz


def compute_ap(recall, precision):
    """AP of one precision-recall curve (1-D arrays, in ranking order) -> (ap, mpre, mrec).  Sentinels 0 / 1 on recall and 1 / 0 on
    precision, the precision envelope taken from the right, then the envelope read at 101 recall points and integrated with the trapezoid
    rule.  (The last point reads the 0 sentinel at recall 1, so a perfect ranking scores 0.995, not 1.)"""
    mrec = np.concatenate(([0.0], recall, [1.0]))
    mpre = np.concatenate(([1.0], precision, [0.0]))
    mpre = np.flip(np.maximum.accumulate(np.flip(mpre)))
    x = np.linspace(0, 1, 101)
    return float(_trapezoid(np.interp(x, mrec, mpre), x)), mpre, mrec


def smooth(y, f=0.05):
    """box filter of fraction f of len(y) (an odd number of taps), the ends held"""
    nf = round(len(y) * f * 2) // 2 + 1
    p = np.ones(nf // 2)
    yp = np.concatenate((p * y[0], y, p * y[-1]), 0)
    return np.convolve(yp, np.ones(nf) / nf, mode="valid")


def ap_per_class(tp, conf, pred_cls, labels, eps=1e-16):
    """tp bool [n, nthr] (true positive at threshold j), conf [n], pred_cls int [n], labels int [num_cls] (ground-truth boxes per class)
    -> (p [num_cls], r [num_cls], f1 [num_cls], ap [num_cls, nthr]), float64.
    Detections are ranked by -conf with a STABLE sort, so equal confidences keep the order they come in (yolov5 calls np.argsort(-conf),
    whose default sort is not stable: there the result at tied confidences is whatever quicksort leaves).  Per class: cumulative TP and
    FP, recall = TP / (labels + eps), precision = TP / (TP + FP), AP per threshold by compute_ap.  P, R and F1 come from the curves of
    threshold 0 resampled on 1000 confidence points, read at the argmax of the smoothed mean F1 over the classes that have labels (the
    classes yolov5 has rows for).  A class without detections or without labels keeps a zero row; nothing divides by zero."""
    tp = np.asarray(tp, dtype=bool)
    tp = tp[:, None] if tp.ndim == 1 else tp
    conf = np.asarray(conf, dtype=np.float64)
    pred_cls = np.asarray(pred_cls)
    labels = np.asarray(labels)
    order = np.argsort(-conf, kind="stable")
    tp, conf, pred_cls = tp[order], conf[order], pred_cls[order]
    nc, nthr = len(labels), tp.shape[1]
    px = np.linspace(0, 1, 1000)
    ap, p, r = np.zeros((nc, nthr)), np.zeros((nc, 1000)), np.zeros((nc, 1000))
    for c in range(nc):
        i = pred_cls == c
        if not i.any() or labels[c] <= 0:
            continue
        tpc = tp[i].cumsum(0)
        fpc = (~tp[i]).cumsum(0)
        recall = tpc / (labels[c] + eps)
        precision = tpc / (tpc + fpc)
        r[c] = np.interp(-px, -conf[i], recall[:, 0], left=0)
        p[c] = np.interp(-px, -conf[i], precision[:, 0], left=1)
        for j in range(nthr):
            ap[c, j] = compute_ap(recall[:, j], precision[:, j])[0]
    f1 = 2 * p * r / (p + r + eps)
    have = labels > 0
    at = int(smooth(f1[have].mean(0), 0.1).argmax()) if have.any() else 0
    return p[:, at], r[:, at], f1[:, at], ap


def fitness(map50, map50_95):
    """yolov5's model-selection score: its weights (0, 0, 0.1, 0.9) on (P, R, mAP@.5, mAP@.5:.95)"""
    return 0.1 * map50 + 0.9 * map50_95
