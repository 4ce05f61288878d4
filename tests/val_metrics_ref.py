"""References for yolov5-style validation scoring (validation.get_metrics, yf_val_match_iouv, metrics.py), none of them importing the package:
  * `process_batch_literal`: yolov5's val.py process_batch (v6.1 on) line by line, torch + numpy, with a stable argsort;
  * `direct_hits` / `direct_records`: the rule as include/yolo_fastest_hip.h states it, one detection at a time in numpy float32;
  * `ap_per_class_loops`: precision, recall and AP with Python loops and its own interpolation, no np.interp / np.trapz;
  * `CASES`: the kernel cases of tests/test_gpu_val_metrics.py, the smallest shapes that can break a 256-wide workgroup."""
import bisect

import numpy as np
import torch

F32 = np.float32
W = 256                                  # val_match_iouv_kernel's workgroup width (csrc/yf_kernels.h: VAL_IOUV_THREADS)
MAX_T = 512                              # VAL_IOUV_MAX_T
IOUV = torch.linspace(0.5, 0.95, 10).numpy().astype(np.float32)


def box_iou(box1, box2, eps=1e-7):
    """yolov5's utils/metrics.py box_iou: box1 [N, 4], box2 [M, 4] -> [N, M], float32"""
    (a1, a2), (b1, b2) = box1.unsqueeze(1).chunk(2, 2), box2.unsqueeze(0).chunk(2, 2)
    inter = (torch.min(a2, b2) - torch.max(a1, b1)).clamp(0).prod(2)
    return inter / ((a2 - a1).prod(2) + (b2 - b1).prod(2) - inter + eps)


def process_batch_literal(det, targets, iouv):
    """det float32 [n, 7] (x1, y1, x2, y2, obj, cls_conf, cls), targets float32 [T, 6] (x1, y1, x2, y2, cls, marker), iouv float32 [nthr]
    -> correct bool [n, nthr].  yolov5's `detections` are (x1, y1, x2, y2, conf, cls) and its `labels` (cls, x1, y1, x2, y2)."""
    det, targets = torch.as_tensor(det), torch.as_tensor(targets)
    targets = targets[targets[:, 5] > 1]
    detections = torch.cat((det[:, :4], det[:, 4:5] * det[:, 5:6], det[:, 6:7]), 1)
    labels = torch.cat((targets[:, 4:5], targets[:, :4]), 1)
    iouv = torch.as_tensor(iouv)
    correct = np.zeros((detections.shape[0], iouv.shape[0])).astype(bool)
    iou = box_iou(labels[:, 1:], detections[:, :4])
    correct_class = labels[:, 0:1] == detections[:, 5]
    for i in range(len(iouv)):
        x = torch.where((iou >= iouv[i]) & correct_class)          # IoU > threshold and classes match
        if x[0].shape[0]:
            matches = torch.cat((torch.stack(x, 1), iou[x[0], x[1]][:, None]), 1).cpu().numpy()   # [label, detect, iou]
            if x[0].shape[0] > 1:
                matches = matches[matches[:, 2].argsort(kind="stable")[::-1]]
                matches = matches[np.unique(matches[:, 1], return_index=True)[1]]
                # matches = matches[matches[:, 2].argsort()[::-1]]
                matches = matches[np.unique(matches[:, 0], return_index=True)[1]]
            correct[matches[:, 1].astype(int), i] = True
    return correct


def ious_of(d, targets):
    """fp32 IoU of one detection row against every target row, the header's operation order; NaN where torch would give NaN"""
    with np.errstate(all="ignore"):
        iw = np.minimum(d[2], targets[:, 2]) - np.maximum(d[0], targets[:, 0])
        ih = np.minimum(d[3], targets[:, 3]) - np.maximum(d[1], targets[:, 1])
        iw[iw < 0] = 0
        ih[ih < 0] = 0
        inter = iw * ih
        a_t = (targets[:, 2] - targets[:, 0]) * (targets[:, 3] - targets[:, 1])
        a_d = F32((d[2] - d[0]) * (d[3] - d[1]))
        return (inter / ((a_t + a_d) - inter + F32(1e-7))).astype(np.float32)


def best_targets(det, targets):
    """-> [(b(k), iou(k, b(k))) or (None, None)] per detection; also whether some detection has two same-class targets at one IoU"""
    det, targets = np.asarray(det, np.float32).reshape(-1, 7), np.asarray(targets, np.float32).reshape(-1, 6)
    out = []
    for d in det:
        b, best = None, None
        if len(targets):
            iou = ious_of(d, targets)
            for t in range(len(targets)):
                if targets[t, 5] > 1 and targets[t, 4] == d[6] and not np.isnan(iou[t]) and (b is None or iou[t] > best):
                    b, best = t, iou[t]
        out.append((b, best))
    return out


def tied(det, targets, floor):
    """the condition process_batch_literal needs: does a detection have two same-class targets at equal fp32 IoU >= floor?"""
    det, targets = np.asarray(det, np.float32).reshape(-1, 7), np.asarray(targets, np.float32).reshape(-1, 6)
    for d in det:
        iou = ious_of(d, targets) if len(targets) else np.zeros(0, np.float32)
        seen = [float(iou[t]) for t in range(len(targets)) if targets[t, 5] > 1 and targets[t, 4] == d[6] and iou[t] >= floor]
        if len(seen) != len(set(seen)):
            return True
    return False


def direct_hits(det, targets, thr):
    """hit masks [n] by the direct definition: candidates per target, the lowest slot wins"""
    bt = best_targets(det, targets)
    hit = np.zeros(len(bt), np.int64)
    for j, th in enumerate(np.asarray(thr, np.float32)):
        winner = {}
        for k, (b, iou) in enumerate(bt):
            if b is not None and iou >= th and b not in winner:
                winner[b] = k
        for k in winner.values():
            hit[k] |= 1 << j
    return hit


def direct_records(det, counts, targets, thr):
    """what yf_val_match_iouv writes for a batch: int32 [total, 4], image then slot order"""
    det = np.asarray(det, np.float32)
    kmax, rows = det.shape[1], []
    for i, count in enumerate(counts):
        n = min(max(int(count), 0), kmax)
        d = det[i, :n]
        hit = direct_hits(d, np.asarray(targets, np.float32)[i], thr)
        rows.append(np.stack((d[:, 4].copy().view(np.int32), d[:, 5].copy().view(np.int32), d[:, 6].astype(np.int32), hit.astype(np.int32)), 1))
    return np.concatenate(rows).reshape(-1, 4)


def _interp(x, xp, fp, left=None):
    """linear interpolation on a non-decreasing xp; at a repeated xp the LAST of the equal points is read, as np.interp does"""
    if x < xp[0]:
        return fp[0] if left is None else left
    if x >= xp[-1]:
        return fp[-1]
    j = bisect.bisect_right(xp, x) - 1
    if xp[j] == x:
        return fp[j]
    return fp[j] + (x - xp[j]) * (fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j])


def compute_ap_loops(recall, precision):
    mrec = [0.0] + [float(v) for v in recall] + [1.0]
    mpre = [1.0] + [float(v) for v in precision] + [0.0]
    for i in range(len(mpre) - 2, -1, -1):
        mpre[i] = max(mpre[i], mpre[i + 1])
    ys = [_interp(i / 100, mrec, mpre) for i in range(101)]
    return sum((ys[i] + ys[i + 1]) / 2 * ((i + 1) / 100 - i / 100) for i in range(100))


def ap_per_class_loops(tp, conf, pred_cls, labels, eps=1e-16):
    """-> (p, r, f1 [num_cls], ap [num_cls, nthr]); ranking: confidence descending, equal confidences in the order given"""
    tp, nc = np.asarray(tp, bool), len(labels)
    nthr = tp.shape[1]
    order = sorted(range(len(conf)), key=lambda i: -float(conf[i]))           # sorted() is stable
    ap = np.zeros((nc, nthr))
    pc, rc = np.zeros((nc, 1000)), np.zeros((nc, 1000))
    for c in range(nc):
        mine = [i for i in order if int(pred_cls[i]) == c]
        if not mine or labels[c] <= 0:
            continue
        for j in range(nthr):
            t = f = 0
            rec, pre = [], []
            for i in mine:
                t, f = t + bool(tp[i, j]), f + (not tp[i, j])
                rec.append(t / (labels[c] + eps))
                pre.append(t / (t + f))
            ap[c, j] = compute_ap_loops(rec, pre)
            if j == 0:
                xs = [-float(conf[i]) for i in mine]
                for q in range(1000):
                    x = -(q / 999)
                    rc[c, q] = _interp(x, xs, rec, left=0.0)
                    pc[c, q] = _interp(x, xs, pre, left=1.0)
    f1 = 2 * pc * rc / (pc + rc + eps)
    have = [c for c in range(nc) if labels[c] > 0]
    at = 0
    if have:
        mean = [sum(f1[c, q] for c in have) / len(have) for q in range(1000)]
        nf = round(1000 * 0.1 * 2) // 2 + 1                                   # yolov5's smooth(y, 0.1): 101 taps, the ends held
        padded = [mean[0]] * (nf // 2) + mean + [mean[-1]] * (nf // 2)
        sm = [sum(padded[q:q + nf]) / nf for q in range(1000)]
        at = max(range(1000), key=lambda q: (sm[q], -q))                      # the first maximum
    return pc[:, at], rc[:, at], f1[:, at], ap


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------

def random_image(rng, n, T, ncls=3, live=0.8):
    """-> det [n, 7], targets [T, 6].  Targets are random boxes, `live` of them with marker 255, the rest 0 or 1; most detections are a
    target's box jittered by up to a fifth of its size (IoUs spread over 0.4 .. 1), some of another class, some anywhere."""
    tg = np.zeros((T, 6), np.float32)
    xy = rng.uniform(0, 250, (T, 2))
    wh = rng.uniform(20, 120, (T, 2))
    tg[:, :2], tg[:, 2:4] = xy, xy + wh
    tg[:, 4] = rng.integers(0, ncls, T)
    tg[:, 5] = np.where(rng.uniform(size=T) < live, 255.0, rng.integers(0, 2, T))
    det = np.zeros((n, 7), np.float32)
    for k in range(n):
        if T and rng.uniform() < 0.85:
            t = int(rng.integers(0, T))
            w, h = tg[t, 2] - tg[t, 0], tg[t, 3] - tg[t, 1]
            det[k, :4] = tg[t, :4] + rng.uniform(-0.2, 0.2, 4) * (w, h, w, h)
            det[k, 6] = tg[t, 4] if rng.uniform() < 0.9 else (tg[t, 4] + 1) % ncls
        else:
            x, y = rng.uniform(0, 250, 2)
            det[k, :4] = (x, y, x + rng.uniform(20, 120), y + rng.uniform(20, 120))
            det[k, 6] = rng.integers(0, ncls)
    det[:, 4], det[:, 5] = rng.uniform(0.001, 1, n), rng.uniform(0.3, 1, n)
    return det, tg


def random_batch(seed, ns, T, kmax=None):
    """images of ns[i] detections -> det [N, kmax, 7] (rows past the count are -7), counts, targets [N, T, 6]"""
    rng = np.random.default_rng(seed)
    kmax = kmax or max(1, max(ns))
    det = np.full((len(ns), kmax, 7), -7.0, np.float32)
    tg = np.zeros((len(ns), T, 6), np.float32)
    for i, n in enumerate(ns):
        d, tg[i] = random_image(rng, n, T)
        det[i, :min(n, kmax)] = d[:kmax]
    return det, list(ns), tg


def _contested(losers_first):
    """one target, three detections over it in three different waves of the workgroup (slots 3, 70 and 200), every other slot far away:
    the winner is slot 3 whichever wave gets to the table first.  `losers_first`: the later slots have the HIGHER IoU (it must not matter)."""
    det = np.zeros((1, W, 7), np.float32)
    det[0, :, :4] = (400, 400, 420, 420)
    det[0, :, 4:6] = 0.5
    boxes = [(10, 10, 50, 48), (10, 10, 50, 49), (10, 10, 50, 50)]
    for slot, box in zip((3, 70, 200), boxes if losers_first else boxes[::-1]):
        det[0, slot, :4] = box
    tg = np.zeros((1, 4, 6), np.float32)
    tg[0, 2] = (10, 10, 50, 50, 0, 255)
    return det, [W], tg


def _two_contest_across_waves():
    """two detections on one target, the winner (slot 1) in wave 0 and the loser (slot 255) in wave 3; a second target has its two
    candidates the other way round in IoU; both targets sit at the ends of the table (index 0 and T - 1)"""
    det = np.zeros((1, W, 7), np.float32)
    det[0, :, :4] = (400, 400, 420, 420)
    det[0, :, 4:6] = 0.5
    det[0, 1, :4], det[0, 255, :4] = (10, 10, 50, 47), (10, 10, 50, 50)
    det[0, 64, :4], det[0, 130, :4] = (100, 100, 160, 160), (100, 100, 160, 150)
    tg = np.zeros((1, 65, 6), np.float32)
    tg[0, 0] = (10, 10, 50, 50, 0, 255)
    tg[0, 64] = (100, 100, 160, 160, 0, 255)
    return det, [W], tg


def _special_values():
    """duplicate targets (tied IoU: the lowest index), a perfect box of the wrong class, markers 0 and 1 over a perfect box, NaN and
    infinite corners in detections and targets"""
    nan, inf = float("nan"), float("inf")
    box = (10, 10, 50, 50)
    rows = [box + (0.9, 0.9, 0), (12, 10, 50, 50, 0.8, 0.9, 0), box + (0.9, 0.8, 1), (nan, 10, 50, 50, 0.7, 0.9, 0), (10, 10, 50, nan, 0.7, 0.8, 0),
            (10, 10, inf, 50, 0.6, 0.9, 0), (-inf, 10, inf, 50, 0.6, 0.8, 0), (-inf, -inf, inf, inf, 0.5, 0.9, 0), (100, 100, 140, 140, 0.5, 0.8, 2),
            (200, 200, 240, 240, 0.4, 0.9, 2), (300, 10, 340, 50, 0.4, 0.8, 0)]
    det = np.tile(np.array(rows, np.float32)[None], (4, 1, 1))
    tg = np.zeros((4, 9, 6), np.float32)
    tg[:, 1] = box + (0, 255)
    tg[:, 3] = box + (0, 255)                       # the duplicate of 1
    tg[:, 4] = box + (2, 255)                       # right box, class 2: detection 2 (class 1) has nothing
    tg[:, 5] = (100, 100, 140, 140, 2, 1)           # marker 1: does not exist
    tg[:, 6] = (200, 200, 240, 240, 2, 0)           # marker 0 neither
    tg[:, 7] = (300, 10, 340, 50, 0, 255)
    tg[1, 1, 2] = inf                               # an infinite target
    tg[2, 1, 0] = nan                               # a NaN target: nobody's best, the duplicate takes over
    tg[3, :, 5] = 1                                 # image 3: no targets at all
    return det, [len(rows)] * 4, tg


def _threshold_cases():
    """a detection and its target whose fp32 IoU (computed here, on the CPU) IS the threshold, then one step above and one below it"""
    det = np.zeros((1, 1, 7), np.float32)
    det[0, 0] = (10, 10, 47, 50, 0.9, 0.9, 0)
    tg = np.zeros((1, 1, 6), np.float32)
    tg[0, 0] = (10, 10, 50, 50, 0, 255)
    iou = ious_of(det[0, 0], tg[0])[0]
    assert 0.9 < iou < 1 and iou.dtype == np.float32
    up, down = np.nextafter(iou, F32(2)), np.nextafter(iou, F32(0))
    return [("iou_is_the_threshold", (det, [1], tg), [iou]), ("threshold_one_step_up", (det, [1], tg), [up]),
            ("threshold_one_step_down", (det, [1], tg), [down]), ("the_three_together", (det, [1], tg), [down, iou, up])]


def _cases():
    out = []
    for n in (W - 1, W, W + 1, 2 * W + 1):
        out.append(("n_%d" % n, random_batch(n, [n, 5], 64), IOUV))
    for T in (0, 1, 63, 64, 65, MAX_T):
        out.append(("T_%d" % T, random_batch(100 + T, [70, 0, 130], T), IOUV))
    out.append(("n_513_T_cap_16_thresholds", random_batch(7, [2 * W + 1], MAX_T), np.linspace(0.2, 0.95, 16).astype(np.float32)))
    out.append(("one_threshold", random_batch(8, [90, 40], 64), [F32(0.5)]))
    out.append(("three_contest_winner_has_lowest_iou", _contested(True), IOUV))
    out.append(("three_contest_winner_has_highest_iou", _contested(False), IOUV))
    out.append(("two_contest_across_waves_targets_at_0_and_T_minus_1", _two_contest_across_waves(), IOUV))
    out.append(("special_values", _special_values(), IOUV))
    out.extend(_threshold_cases())
    out.append(("kmax_below_a_count", random_batch(9, [40, 12, 33], 64, kmax=20), IOUV))
    det, _, tg = random_batch(10, [6, 6, 6, 6, 6], 64)
    out.append(("negative_and_huge_counts", (det, [9, 2, -3, 2 ** 31 - 1, 4], tg), IOUV))
    return out


CASES = _cases()
