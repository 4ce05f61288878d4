"""ORACLE (test infrastructure, not product): CPU restatement of the reference's TRAINING-time loss of one head
(first slice) and, through torch autograd on this restatement, its gradient with respect to the head tensor.

Follows (file:line under the reference repo)
    src/model_training/loss/yolo_loss.py   YOLOLossV3.forward with targets :48-97, get_target :144-196
    src/model_training/utils/general.py    bbox_iou :29-52 (x1y1x2y2 branch, +1 pixel convention)
    src/model_training/_config.py          train_params.IOU_loss_thre = 0.5 (:45)

Parity pin: tests/test_oracle_golden.py checks this file against tests/golden/golden_loss_256.npz, produced by
tests/golden/make_golden.py (main_loss) by importing and running the reference's own YOLOLossV3 with targets and calling
backward() on its total loss.
"""
import math

import numpy as np
import torch
import torch.nn as nn


def _bbox_iou(box1, box2):  # general.py:29-52
    ix1 = torch.max(box1[:, 0], box2[:, 0]); iy1 = torch.max(box1[:, 1], box2[:, 1])
    ix2 = torch.min(box1[:, 2], box2[:, 2]); iy2 = torch.min(box1[:, 3], box2[:, 3])
    inter = torch.clamp(ix2 - ix1 + 1, min=0) * torch.clamp(iy2 - iy1 + 1, min=0)
    a1 = (box1[:, 2] - box1[:, 0] + 1) * (box1[:, 3] - box1[:, 1] + 1)
    a2 = (box2[:, 2] - box2[:, 0] + 1) * (box2[:, 3] - box2[:, 1] + 1)
    return inter / (a1 + a2 - inter + 1e-16)


def get_target(target, anchors, in_w, in_h, ignore_threshold, num_classes=3):
    """yolo_loss.py:144-196.  target float32 [bs, T, 6]; anchors: list of (w, h) Python floats in feature-map units."""
    bs, A = target.size(0), len(anchors)
    mask = torch.zeros(bs, A, in_h, in_w); noobj_mask = torch.ones(bs, A, in_h, in_w)
    tx = torch.zeros(bs, A, in_h, in_w); ty = torch.zeros(bs, A, in_h, in_w)
    tw = torch.zeros(bs, A, in_h, in_w); th = torch.zeros(bs, A, in_h, in_w)
    tcls = torch.zeros(bs, A, in_h, in_w, num_classes)
    for b in range(bs):
        for t in range(target.shape[1]):
            if target[b, t, 5] < 1:
                break
            gx = target[b, t, 0] * in_w; gy = target[b, t, 1] * in_h
            gw = target[b, t, 2] * in_w; gh = target[b, t, 3] * in_h
            if gw <= 0 or gh <= 0:
                continue
            gi, gj = int(gx), int(gy)
            gt_box = torch.FloatTensor(np.array([0.0, 0.0, gw, gh], dtype=np.float32)).unsqueeze(0)
            anchor_shapes = torch.FloatTensor(np.concatenate((np.zeros((A, 2)), np.array(anchors)), 1))
            anch_ious = _bbox_iou(gt_box, anchor_shapes)
            noobj_mask[b, anch_ious > ignore_threshold, gj, gi] = 0
            best_n = int(np.argmax(anch_ious))
            mask[b, best_n, gj, gi] = 1
            tx[b, best_n, gj, gi] = gx - gi
            ty[b, best_n, gj, gi] = gy - gj
            tw[b, best_n, gj, gi] = math.log(gw / anchors[best_n][0] + 1e-16)
            th[b, best_n, gj, gi] = math.log(gh / anchors[best_n][1] + 1e-16)
            tcls[b, best_n, gj, gi, int(target[b, t, 4])] = 1
    return mask, noobj_mask, tx, ty, tw, th, tcls


def loss_head(x, targets, anchors, num_classes, input_shape, ignore_threshold=0.5):
    """yolo_loss.py:48-97.  x float32 [bs, A*(5+C), h, w] (may require grad) -> (loss tensor, x, y, w, h, conf, cls as floats)."""
    bs, _, in_h, in_w = x.shape
    A = len(anchors)
    stride_h, stride_w = input_shape[0] / in_h, input_shape[1] / in_w
    scaled = [(a_w / stride_w, a_h / stride_h) for a_w, a_h in anchors]
    p = x.view(bs, A, 5 + num_classes, in_h, in_w).permute(0, 1, 3, 4, 2).contiguous()
    sx, sy = torch.sigmoid(p[..., 0]), torch.sigmoid(p[..., 1])
    w, h = p[..., 2], p[..., 3]
    conf = torch.sigmoid(p[..., 4])
    pred_cls = torch.sigmoid(p[..., 5:])
    mask, noobj_mask, tx, ty, tw, th, tcls = get_target(targets, scaled, in_w, in_h, ignore_threshold, num_classes)
    bce, mse = nn.BCELoss(), nn.MSELoss()
    loss_x = bce(sx * mask, tx * mask); loss_y = bce(sy * mask, ty * mask)
    loss_w = mse(w * mask, tw * mask); loss_h = mse(h * mask, th * mask)
    loss_conf = bce(conf * mask, mask) + 0.5 * bce(conf * noobj_mask, noobj_mask * 0.0)
    loss_cls = bce(pred_cls[mask == 1], tcls[mask == 1])
    loss = loss_x * 2.5 + loss_y * 2.5 + loss_w * 2.5 + loss_h * 2.5 + loss_conf * 1.0 + loss_cls * 1.0
    return loss, loss_x.item(), loss_y.item(), loss_w.item(), loss_h.item(), loss_conf.item(), loss_cls.item()


def loss_and_grad(x, targets, anchors, num_classes, input_shape, ignore_threshold=0.5):
    """-> (float32[7] losses, grad of the total loss with respect to x, like x)."""
    x = x.detach().clone().requires_grad_(True)
    out = loss_head(x, targets, anchors, num_classes, input_shape, ignore_threshold)
    out[0].backward()
    return np.array([out[0].item()] + list(out[1:]), np.float32), x.grad.detach()


# ---- float64 model of the device's launch group (tests/loss_cases.py, tests/test_cpu_loss_cases.py, tests/test_gpu_loss.py) ----

def drop_unindexable(target, in_w, in_h, num_classes):
    """The targets the reference cannot index: cell (int(x * in_w), int(y * in_h)) outside the map or class int(class) outside
    0 .. num_classes-1, negative indices included (the reference wraps those round; yf_train_head_loss_ex counts them all in losses[7] and
    skips them whole, include/yolo_fastest_hip.h).  -> (a copy in which each such target has zero width, which get_target :166 skips, their
    number).  The products are torch float32 ones, as in get_target."""
    t = target.clone()
    count = 0
    for b in range(t.size(0)):
        for k in range(t.shape[1]):
            if t[b, k, 5] < 1:
                break
            if t[b, k, 2] * in_w <= 0 or t[b, k, 3] * in_h <= 0:
                continue
            gi, gj, c = int(t[b, k, 0] * in_w), int(t[b, k, 1] * in_h), int(t[b, k, 4])
            if gi < 0 or gi >= in_w or gj < 0 or gj >= in_h or c < 0 or c >= num_classes:
                count += 1
                t[b, k, 2] = 0.0
    return t, count


def scaled_anchors(anchors, input_shape, in_h, in_w):
    """yolo_loss.py:52-56: the head's anchors in feature-map units, Python doubles."""
    stride_h, stride_w = input_shape[0] / in_h, input_shape[1] / in_w
    return [(a_w / stride_w, a_h / stride_h) for a_w, a_h in anchors]


LOSS_NAMES = ("total", "x", "y", "w", "h", "conf", "cls")
GRAD_KINDS = ("x", "y", "w", "h", "conf_pos", "conf_noobj", "cls", "box_off", "conf_ignored", "cls_off")


def grad_kinds(planes, num_classes):
    """{kind: bool [N, A, 5 + C, fh, fw]} -- the term kinds a gradient is judged by.  x, y, w, h, cls: that channel at positive cells (mask 1);
    conf_pos: the confidence at positive cells; conf_noobj: at cells with mask 0 and noobj_mask 1; and the three kinds whose gradient is zero
    in exact arithmetic: box_off / cls_off (box and class channels at non-positive cells), conf_ignored (mask 0, noobj_mask 0)."""
    m, nm = planes[0].numpy() == 1, planes[1].numpy() == 1
    k = {n: np.zeros(m.shape[:2] + (5 + num_classes,) + m.shape[2:], bool) for n in GRAD_KINDS}
    for i, n in enumerate(("x", "y", "w", "h")):
        k[n][:, :, i] = m
    k["box_off"][:, :, 0:4] = ~m[:, :, None]
    k["conf_pos"][:, :, 4] = m
    k["conf_noobj"][:, :, 4] = ~m & nm
    k["conf_ignored"][:, :, 4] = ~m & ~nm
    k["cls"][:, :, 5:] = m[:, :, None]
    k["cls_off"][:, :, 5:] = ~m[:, :, None]
    return k


def _model_core(sig, v, m, nm, tx, ty, tw, th, tc, C):
    """terms, losses and gradient from the (already rounded) sigmoids `sig` and the raw logits `v`, both float64 [bs, A, 5 + C, h, w]"""
    px, py, pc, pk = sig[:, :, 0], sig[:, :, 1], sig[:, :, 4], sig[:, :, 5:]
    w, h = v[:, :, 2], v[:, :, 3]

    def bce(p, t):
        return -(t * np.maximum(np.log(p), -100.0) + (1.0 - t) * np.maximum(np.log(1.0 - p), -100.0))

    def dbce(p, t):
        return (p - t) / np.maximum((1.0 - p) * p, 1e-12)
    E = float(m.size)
    n_pos = float(m.sum())
    pos = m == 1
    terms = dict(x=bce(px * m, tx * m), y=bce(py * m, ty * m), w=(w * m - tw * m) ** 2, h=(h * m - th * m) ** 2,
                 conf_obj=bce(pc * m, m), conf_noobj=bce(pc * nm, nm * 0.0), cls=bce(pk, tc) * pos[:, :, None])
    g = np.zeros(v.shape, np.float64)
    g[:, :, 0] = 2.5 / E * dbce(px * m, tx * m) * m * (1.0 - px) * px
    g[:, :, 1] = 2.5 / E * dbce(py * m, ty * m) * m * (1.0 - py) * py
    g[:, :, 2] = 2.5 / E * 2.0 * (w * m - tw * m) * m
    g[:, :, 3] = 2.5 / E * 2.0 * (h * m - th * m) * m
    g[:, :, 4] = (dbce(pc * m, m) * m + 0.5 * dbce(pc * nm, 0.0) * nm) * (1.0 - pc) * pc / E
    if n_pos:
        g[:, :, 5:] = dbce(pk, tc) * (1.0 - pk) * pk / (C * n_pos) * pos[:, :, None]
    return terms, g, E, n_pos


def _combine(sums, E, C, n_pos):
    """per-term sums -> the seven losses, combined like yolo_loss.py:90-92"""
    lx, ly, lw, lh = (sums[k] / E for k in "xywh")
    lconf = sums["conf_obj"] / E + 0.5 * (sums["conf_noobj"] / E)
    lcls = sums["cls"] / (C * n_pos) if n_pos else float("nan")
    return np.array([2.5 * (lx + ly + lw + lh) + lconf + lcls, lx, ly, lw, lh, lconf, lcls], np.float64)


def loss_model64(x, targets, anchors, num_classes, input_shape, ignore_threshold=0.5, planes=None, round_p=True):
    """"float64 that rounds where fp32 must": the launch group of yf_train_head_loss_ex with every operation in float64 EXCEPT
      * get_target, which stays the reference's fp32 arithmetic (compared bit for bit; `planes` = a get_target result to use instead), and
      * the sigmoid: p = float32(sigmoid64(logit)).  The reference's BCE is a function of the ROUNDED p: once 1 - p rounds to 0 (logit >= 17)
        log(1 - p) is the clamp -100, which a plain float64 sigmoid never reaches.
    After that torch's formulas with torch's clamps (log >= -100; BCE backward's denominator >= 1e-12) and the reference's combination
    2.5 (x + y + w + h) + conf_obj + 0.5 conf_noobj + cls (yolo_loss.py:78-92).
    -> dict: planes, terms {name: float64 per-cell values}, losses float64 [7] (LOSS_NAMES; nan cls / total without a positive cell, like
    the mean of an empty tensor), grad float64 like x, n_pos, and what ONE float32 step of every sigmoid is worth: p_ulp_losses [7] (the sum
    over the cells of the larger change of each term under p -> the float32 above / below it) and p_ulp_grad (the same per gradient
    element).  A sigmoid that is exactly 0 or 1 is not stepped: outside (15, 18) any float32 sigmoid saturates where this one does.
    round_p=False leaves the sigmoid in float64: plain float64 throughout, what torch autograd of loss_head in float64 computes (the pin
    of every formula here, tests/test_cpu_loss_cases.py)."""
    xs = np.asarray(x.detach().numpy() if torch.is_tensor(x) else x)
    bs, _, in_h, in_w = xs.shape
    A, C = len(anchors), num_classes
    if planes is None:
        planes = get_target(targets, scaled_anchors(anchors, input_shape, in_h, in_w), in_w, in_h, ignore_threshold, C)
    m, nm, tx, ty, tw, th = (a.numpy().astype(np.float64) for a in planes[:6])
    tc = planes[6].numpy().astype(np.float64).transpose(0, 1, 4, 2, 3)            # [bs, A, C, h, w]
    v = xs.reshape(bs, A, 5 + C, in_h, in_w).astype(np.float64)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        sig32 = (1.0 / (1.0 + np.exp(-v))).astype(np.float32)
        terms, g, E, n_pos = _model_core(sig32.astype(np.float64) if round_p else 1.0 / (1.0 + np.exp(-v)), v, m, nm, tx, ty, tw, th, tc, C)
        losses = _combine({k: t.sum() for k, t in terms.items()}, E, C, n_pos)
        free = (sig32 > 0) & (sig32 < 1)
        dterm = {k: np.zeros_like(t) for k, t in terms.items()}
        dg = np.zeros_like(g)
        for toward in (np.float32(2), np.float32(-1)):
            step = np.where(free, np.nextafter(sig32, toward), sig32).astype(np.float64)
            t2, g2, _, _ = _model_core(step, v, m, nm, tx, ty, tw, th, tc, C)
            dterm = {k: np.maximum(dterm[k], np.abs(t2[k] - terms[k])) for k in terms}
            dg = np.maximum(dg, np.abs(g2 - g))
        p_ulp_losses = np.nan_to_num(_combine({k: t.sum() for k, t in dterm.items()}, E, C, n_pos), nan=0.0)
    return dict(planes=planes, terms=terms, losses=losses, grad=g.reshape(xs.shape), n_pos=int(n_pos), p_ulp_losses=p_ulp_losses,
                p_ulp_grad=dg.reshape(xs.shape))
