"""The IoU-family box loss of one head (`yf_train_head_loss_box`: loss_cells_kernel<GRAD, true>, loss_final_kernel in
csrc/yf_loss_kernels.hip), stated once as a dtype-generic torch function, with its case table and its comparator.  Shared by
tests/test_cpu_box_loss.py (the definition alone) and tests/test_gpu_box_loss.py (the kernels).

THE DEFINITION (`box_values`), per positive cell, in feature-map units relative to the cell's corner:
  predicted box  px = sigmoid(t0), py = sigmoid(t1), pw = exp(clamp(t2, -10, 10)) * aw, ph = exp(clamp(t3, -10, 10)) * ah
  target box     tx, ty (get_target's float32 planes), gw = float32(w * fw), gh = float32(h * fh) of the target that wrote tx
  value          GIoU, DIoU or CIoU of the two (yolov5's bbox_iou, eps = 1e-7; CIoU's alpha is a constant in the backward)
  box            (1 / E) * sum over the positive cells of (1 - value), E = N * A * fh * fw
  total          lambda_box * box + conf + cls, conf and cls the reference's (oracle/loss_oracle.py)

MODEL: `box_values` in float64 with autograd on the float32 logits, anchors and planes widened to double; conf, cls and the gradient of
channels 4.. from oracle.loss_oracle.loss_model64.  TWIN: the same function in float32 with autograd, what a torch user would have computed;
conf and cls from loss_cases.reference's twin.

CASES: every case of loss_cases.cases() plus, on a 4x6 map with N <= 2 (`added_cases`):
  disjoint       tiny boxes in opposite corners of one cell: iou = 0, the gradient comes from the enclosing box / centre distance alone
  pred_inside    the predicted box strictly inside the target
  target_inside  the target strictly inside the predicted box
  aspect         equal centres, crossed shapes: rho2 = 0, CIoU's v is the only thing that separates it from DIoU
  clamp          w / h logits of 10 and -10 exactly, one float32 step inside and outside each, +-12, 80, -1000
  last_wins      two targets of different size in one cell with one best anchor: gw, gh are the LAST one's, like tx
  match          logits that invert the target: value >= 1 - 1e-5; the boxes' corners tie in exact arithmetic, where autograd's
                 subgradient is a convention, so it is judged on losses and finiteness only (`LOSSES_ONLY`)

THE COMPARATOR (`judge`), loss_cases.py's ratio and floors:
  losses   total, box, conf, cls: |dev - m64| <= max(3 |twin - m64|, 8 float32 ulps of |m64|); NaN exactly where the model has NaN;
           d_losses[2..4] exactly 0; [7] exact.
  grad     kind `box` (channels 0..3 at positive cells): max|dev - m64| <= max(3 max|twin - m64|, 4 float32 ulps of the kind's max|m64|);
           conf_pos, conf_noobj, cls the same against loss_model64; box_off, conf_ignored, cls_off exactly zero.
No bound comes from what the device computes.
"""
import math

import numpy as np
import torch

import loss_cases as lc
from oracle import loss_oracle as lo

KINDS = ("giou", "diou", "ciou")
KIND_ID = {"giou": 1, "diou": 2, "ciou": 3}
WH_CLAMP = 10.0
EPS = 1e-7
LAMBDA_BOX = 5.0
LOSS_NAMES = ("total", "box", "conf", "cls")
LOSS_INDEX = (0, 1, 5, 6)
DEFECTS = ("alpha_grad", "npos_norm", "clamp_passthrough", "gw_first", "corner_w")
LOSSES_ONLY = ("match",)
F32 = np.float32


def iou_family(px, py, pw, ph, tx, ty, gw, gh, kind, defect=None):
    """GIoU / DIoU / CIoU of box 1 = (px, py, pw, ph) against box 2 = (tx, ty, gw, gh), centre and size; tensors of one dtype"""
    half = 1.0 if defect == "corner_w" else 0.5
    b1x1, b1x2, b1y1, b1y2 = px - pw * half, px + pw * half, py - ph * half, py + ph * half
    b2x1, b2x2, b2y1, b2y2 = tx - gw * half, tx + gw * half, ty - gh * half, ty + gh * half
    inter = (torch.min(b1x2, b2x2) - torch.max(b1x1, b2x1)).clamp(min=0) * (torch.min(b1y2, b2y2) - torch.max(b1y1, b2y1)).clamp(min=0)
    union = pw * ph + gw * gh - inter + EPS
    iou = inter / union
    cw = torch.max(b1x2, b2x2) - torch.min(b1x1, b2x1)
    ch = torch.max(b1y2, b2y2) - torch.min(b1y1, b2y1)
    if kind == "giou":
        c_area = cw * ch + EPS
        return iou - (c_area - union) / c_area
    c2 = cw ** 2 + ch ** 2 + EPS
    rho2 = ((b2x1 + b2x2 - b1x1 - b1x2) ** 2 + (b2y1 + b2y2 - b1y1 - b1y2) ** 2) / 4
    if kind == "diou":
        return iou - rho2 / c2
    assert kind == "ciou"
    v = (4 / math.pi ** 2) * (torch.atan(gw / (gh + EPS)) - torch.atan(pw / (ph + EPS))) ** 2
    alpha = v / (v - iou + 1 + EPS)
    if defect != "alpha_grad":
        alpha = alpha.detach()
    return iou - (rho2 / c2 + v * alpha)


def box_values(t, anc, tgt, kind, defect=None):
    """t [P, 4] logits, anc [P, 2] anchors (feature-map units), tgt [P, 4] = tx, ty, gw, gh -> value [P]"""
    px, py = torch.sigmoid(t[:, 0]), torch.sigmoid(t[:, 1])
    cl = t[:, 2:4].clamp(-WH_CLAMP, WH_CLAMP)
    if defect == "clamp_passthrough":
        cl = t[:, 2:4] + (cl - t[:, 2:4]).detach()
    wh = torch.exp(cl) * anc
    return iou_family(px, py, wh[:, 0], wh[:, 1], tgt[:, 0], tgt[:, 1], tgt[:, 2], tgt[:, 3], kind, defect)


def size_planes(clean, anc32, fw, fh, first=False):
    """gw, gh float32 [N, A, fh, fw]: float32(w * fw), float32(h * fh) of the target that wrote the cell's tx (the last one; `first`: the
    planted defect).  `clean`: targets without those the reference cannot index (loss_oracle.drop_unindexable)."""
    t = np.asarray(clean, np.float32)
    N, A = t.shape[0], len(anc32)
    pw, ph = np.zeros((N, A, fh, fw), np.float32), np.zeros((N, A, fh, fw), np.float32)
    seen = set()
    for b in range(N):
        for k in range(t.shape[1]):
            if t[b, k, 5] < 1:
                break
            gx, gy, gw, gh = t[b, k, 0] * F32(fw), t[b, k, 1] * F32(fh), t[b, k, 2] * F32(fw), t[b, k, 3] * F32(fh)
            if gw <= 0 or gh <= 0:
                continue
            key = (b, int(np.argmax(lc.iou32(gw, gh, anc32[:, 0], anc32[:, 1]))), int(gy), int(gx))
            if not (first and key in seen):
                pw[key], ph[key] = gw, gh
            seen.add(key)
    return pw, ph


# ---- the cases ----

def _added(name, targets, why, fill):
    """a 4x6 map of the stride-16 head, 3 anchors, 3 classes; `fill(i, tx, ty, gw, gh, aw, ah) -> (t0, t1, t2, t3)` per positive cell i"""
    N, T = targets.shape[:2]
    c = lc._case(name, 7000 + len(name), N, 3, 3, 4, 6, 64, 96, T, lc.ANC_LARGE, targets, why)
    anc = lc.anchors32(c)
    planes = lo.get_target(torch.from_numpy(c.targets), lo.scaled_anchors(c.anchors, (c.H, c.W), c.fh, c.fw), c.fw, c.fh, lc.THRES, c.C)
    gw, gh = size_planes(c.targets, anc, c.fw, c.fh)
    x = c.logits.reshape(N, 3, 8, 4, 6)
    for i, (n, a, j, k) in enumerate(np.argwhere(planes[0].numpy() == 1)):
        x[n, a, 0:4, j, k] = np.asarray(fill(i, float(planes[2][n, a, j, k]), float(planes[3][n, a, j, k]), float(gw[n, a, j, k]),
                                             float(gh[n, a, j, k]), float(anc[a, 0]), float(anc[a, 1])), np.float32)
    return c


def _logit(p):
    return math.log(p / (1.0 - p))


def _rows(rows, N=1):
    T = max(len(r) for r in rows)
    t = np.zeros((N, T, 6), np.float32)
    for n, r in enumerate(rows):
        for k, (x, y, w, h, c) in enumerate(r):
            t[n, k] = (x, y, w, h, c, 255.0)
    return t


def _clamp_values():
    ten = F32(10)
    return [ten, np.nextafter(ten, F32(0)), np.nextafter(ten, F32(99)), -ten, np.nextafter(-ten, F32(0)), np.nextafter(-ten, F32(-99)),
            F32(12), F32(-12), F32(80), F32(-1000)]


def build_added():
    out = []
    # (gi + 0.25) / 6 and (gj + 0.25) / 4 keep the cell's offset away from 0.5, so that no corner of a sigmoid(0) box ties
    out.append(_added("disjoint", _rows([[(1.9 / 6, 2.9 / 4, 0.05 / 6, 0.04 / 4, 1)], [(4.85 / 6, 0.9 / 4, 0.03 / 6, 0.06 / 4, 0)]], 2),
                      "tiny boxes in opposite corners of one cell, iou = 0",
                      lambda i, tx, ty, gw, gh, aw, ah: (_logit(0.1), _logit(0.12), math.log(0.05 / aw), math.log(0.06 / ah))))
    out.append(_added("pred_inside", _rows([[(2.4 / 6, 1.6 / 4, 0.5, 0.6, 2)], [(3.3 / 6, 2.45 / 4, 0.4, 0.7, 1)]], 2),
                      "the predicted box strictly inside the target",
                      lambda i, tx, ty, gw, gh, aw, ah: (_logit(tx + 0.05), _logit(ty - 0.04), math.log(0.3 * gw / aw), math.log(0.5 * gh / ah))))
    out.append(_added("target_inside", _rows([[(2.4 / 6, 1.6 / 4, 0.05, 0.08, 2)], [(3.3 / 6, 2.45 / 4, 0.06, 0.05, 1)]], 2),
                      "the target strictly inside the predicted box",
                      lambda i, tx, ty, gw, gh, aw, ah: (_logit(tx - 0.03), _logit(ty + 0.04), math.log(3.1 * gw / aw), math.log(2.3 * gh / ah))))
    out.append(_added("aspect", _rows([[(1.5 / 6, 1.5 / 4, 0.5, 0.1875, 0)]]),
                      "equal centres (tx = ty = 0.5 exactly, logits 0), crossed shapes",
                      lambda i, tx, ty, gw, gh, aw, ah: (0.0, 0.0, math.log(0.3 * gw / aw), math.log(3.7 * gh / ah))))
    v = _clamp_values()
    rows = [[((k + 0.3) / 6, (n * 2 + 0.7) / 4, 0.2 + 0.02 * k, 0.3 - 0.02 * k, k % 3) for k in range(5)] for n in range(2)]
    out.append(_added("clamp", _rows(rows, 2), "w / h logits at +-10 exactly, one float32 step inside and outside, +-12, 80, -1000",
                      lambda i, tx, ty, gw, gh, aw, ah: (0.3 * i - 1.2, 1.1 - 0.25 * i, v[i], v[(i + 3) % 10])))
    out.append(_added("last_wins", _rows([[(2.2 / 6, 1.7 / 4, 0.30, 0.45, 0), (2.6 / 6, 1.3 / 4, 0.36, 0.50, 1)]]),
                      "two targets of different size in one cell with one best anchor: the last one's tx, ty, gw, gh",
                      lambda i, tx, ty, gw, gh, aw, ah: (0.4, -0.3, 0.2, -0.1)))
    out.append(_added("match", _rows([[(2.3 / 6, 1.6 / 4, 0.2, 0.3, 2), (4.7 / 6, 3.2 / 4, 0.5, 0.25, 0)], [(0.6 / 6, 0.4 / 4, 0.1, 0.6, 1)]], 2),
                      "logits that invert the target: value >= 1 - 1e-5",
                      lambda i, tx, ty, gw, gh, aw, ah: (_logit(tx), _logit(ty), math.log(gw / aw), math.log(gh / ah))))
    return out


_built = {}


def added_cases():
    if "added" not in _built:
        _built["added"] = build_added()
    return _built["added"]


def cases():
    return lc.cases() + added_cases()


def judged_cases():
    return [c for c in cases() if c.logit_set != "band"]


def case_by_name(name):
    return {c.name: c for c in cases()}[name]


# ---- model and twin of a case ----

def positives(case, ref=None):
    """-> (index arrays n, a, j, k of the positive cells in cell order, gw plane, gh plane)"""
    ref = ref or lc.reference(case)
    gw, gh = size_planes(ref["clean"].numpy(), lc.anchors32(case), case.fw, case.fh)
    mask = ref["planes"][0].numpy() == 1
    assert np.array_equal(mask, gw > 0) and np.array_equal(mask, gh > 0)
    return np.nonzero(mask), gw, gh


def head_box(case, kind, dtype, defect=None, logits=None):
    """-> (box = (1 / E) sum (1 - value) as a 0-dim tensor of `dtype` (float64: a plain 0.0 sum without positives), its gradient like the
    logits as float64 numpy, the values [P] as float64 numpy)"""
    ref = lc.reference(case)
    idx, gw, gh = positives(case, ref)
    if defect == "gw_first":
        gw, gh = size_planes(ref["clean"].numpy(), lc.anchors32(case), case.fw, case.fh, first=True)
    n, a, j, k = (torch.from_numpy(i) for i in idx)
    x = torch.from_numpy(case.logits if logits is None else logits).to(dtype).requires_grad_(True)
    p = x.view(case.N, case.A, 5 + case.C, case.fh, case.fw)
    t = p[n, a, :, j, k][:, 0:4]
    anc = torch.from_numpy(lc.anchors32(case)).to(dtype)[a]
    tgt = torch.stack([ref["planes"][2][n, a, j, k], ref["planes"][3][n, a, j, k], torch.from_numpy(gw)[n, a, j, k],
                       torch.from_numpy(gh)[n, a, j, k]], 1).to(dtype)
    val = box_values(t, anc, tgt, kind, defect)
    E = case.N * case.A * case.fh * case.fw
    box = (1.0 - val).sum() / (len(val) if defect == "npos_norm" and len(val) else E)
    box.backward()
    return box.detach(), x.grad.double().numpy(), val.detach().double().numpy()


_refs = {}


def reference(case, kind, lambda_box=LAMBDA_BOX, defect=None):
    """-> dict: losses float64 [7] = total, box, 0, 0, 0, conf, cls of the model; grad float64 like the logits; twin_losses float32 [7];
    twin_grad; kinds {name: bool mask like the logits}; values float64 [P]; gw, gh planes.  Cached (without a defect)."""
    key = (case.name, kind, lambda_box)
    if defect is None and key in _refs:
        return _refs[key]
    ref = lc.reference(case)
    m = ref["m64"]
    box, gbox, values = head_box(case, kind, torch.float64, defect)
    losses = np.array([lambda_box * float(box) + m["losses"][5] + m["losses"][6], float(box), 0.0, 0.0, 0.0, m["losses"][5], m["losses"][6]])
    shape5 = (case.N, case.A, 5 + case.C, case.fh, case.fw)
    grad = m["grad"].reshape(shape5).copy()
    grad[:, :, 0:4] = lambda_box * gbox.reshape(shape5)[:, :, 0:4]
    tbox, tgbox, _ = head_box(case, kind, torch.float32)
    tl = ref["twin_losses"]
    ttotal = torch.tensor(lambda_box, dtype=torch.float32) * tbox + torch.tensor(tl[5]) + torch.tensor(tl[6])
    twin_losses = np.array([float(ttotal), float(tbox), 0.0, 0.0, 0.0, tl[5], tl[6]], np.float32)
    twin_grad = ref["twin_grad"].reshape(shape5).astype(np.float64)
    twin_grad[:, :, 0:4] = (np.float32(lambda_box) * tgbox.astype(np.float32)).reshape(shape5)[:, :, 0:4]
    k0 = ref["kinds"]
    kinds = {"box": k0["x"] | k0["y"] | k0["w"] | k0["h"]}
    kinds.update({n: k0[n] for n in ("conf_pos", "conf_noobj", "cls", "box_off", "conf_ignored", "cls_off")})
    _, gw, gh = positives(case, ref)
    out = dict(losses=losses, grad=grad.reshape(case.logits.shape), twin_losses=twin_losses, twin_grad=twin_grad.reshape(case.logits.shape),
               kinds=kinds, values=values, gw=gw, gh=gh, counted=ref["counted"], n_pos=m["n_pos"])
    if defect is None:
        _refs[key] = out
    return out


def planes_to_dense(case):
    """float32 [8 + C, E]: get_target's planes, then gw, gh -- the layout behind the box workspace's 16 doubles"""
    ref = lc.reference(case)
    _, gw, gh = positives(case, ref)
    return np.concatenate([lc.planes_to_dense(ref["planes"]), gw.reshape(1, -1), gh.reshape(1, -1)]).astype(np.float32)


# ---- the comparator ----

def judge(case, kind, losses8, grad=None, lambda_box=LAMBDA_BOX, ref=None):
    """losses8: the eight float32 of d_losses; grad like the logits or None -> loss_cases.Report"""
    ref = ref or reference(case, kind, lambda_box)
    rep = lc.Report(case)
    if float(losses8[7]) != float(ref["counted"]):
        rep.failures.append("%s losses[7] = %r, want %d" % (case.name, float(losses8[7]), ref["counted"]))
    if any(float(losses8[i]) != 0.0 for i in (2, 3, 4)):
        rep.failures.append("%s losses[2..4] = %r, want exact zeros" % (case.name, [float(v) for v in losses8[2:5]]))
    if case.logit_set == "band":
        fin = [math.isfinite(float(v)) for v in losses8[:7]]
        ok = all(fin[1:6]) and (fin[0] and fin[6]) != (ref["n_pos"] == 0) and (grad is None or bool(np.isfinite(grad).all()))
        if not ok:
            rep.failures.append("%s: a loss or gradient of the band case is not finite (or not the documented NaN): %r" % (case.name, list(losses8)))
        return rep
    for name, i in zip(LOSS_NAMES, LOSS_INDEX):
        d, w, t = float(losses8[i]), float(ref["losses"][i]), float(ref["twin_losses"][i])
        if math.isnan(w):
            rep.add("loss " + name, float("nan"), float("nan"), float("nan"), math.isnan(d))
            continue
        bound = max(lc.ACCURACY_RATIO * abs(t - w), lc.LOSS_ULPS * lc.ulp32(w))
        rep.add("loss " + name, abs(d - w), abs(t - w), bound, math.isfinite(d) and abs(d - w) <= bound)
    if grad is None:
        return rep
    if case.name in LOSSES_ONLY:
        if not np.isfinite(grad).all():
            rep.failures.append("%s: a gradient element is not finite" % case.name)
        return rep
    shape = ref["kinds"]["box"].shape
    g, w, t = (np.asarray(a, np.float64).reshape(shape) for a in (grad, ref["grad"], ref["twin_grad"]))
    for name, sel in ref["kinds"].items():
        if not sel.any():
            continue
        top = np.abs(w[sel]).max()
        if top == 0:
            rep.add("grad " + name, float(np.abs(np.nan_to_num(g[sel], nan=np.inf)).max()), float(np.abs(t[sel]).max()), 0.0, bool((g[sel] == 0).all()))
            continue
        d, dt = np.abs(g[sel] - w[sel]).max(), np.abs(t[sel] - w[sel]).max()
        bound = max(lc.ACCURACY_RATIO * dt, lc.GRAD_ULPS * lc.ulp32(top))
        rep.add("grad " + name, float(d), float(dt), bound, bool(np.isfinite(g[sel]).all() and d <= bound))
    return rep
