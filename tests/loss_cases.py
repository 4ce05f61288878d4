"""Case table and comparator for the training loss of one head (`yf_train_head_loss_ex`: loss_init_kernel, loss_targets_kernel,
loss_cells_kernel<GRAD>, loss_final_kernel in csrc/yf_loss_kernels.hip).  Shared by tests/test_cpu_loss_cases.py (the oracle alone: every
case has the property it names, the fp32 twin stays inside the floors, every planted defect is rejected) and tests/test_gpu_loss.py (the
kernels).  Everything is seeded.

A case is `Case(name, N, A, C, fh, fw, H, W, T, anchors, targets, logits, why)` plus `logit_set` ("M", "S" or "band") and `counted`, the
number of targets the reference cannot index (cell outside the map, class outside 0 .. C-1).

GEOMETRY: the smallest shapes that switch something.  E = N*A*fh*fw of 3, 15, 16, 17 (loss_init_kernel clears its 16 accumulators with
the first 16 threads of block 0, whatever E is) and 255, 256, 257 (one 256-thread workgroup, exactly one, two); maps of 1x1, 3x5 (odd),
4x6, 8x10, 16x20; N of 1, 2, 64, 65, 130 (loss_targets_kernel: one thread per image in 64-thread workgroups); 1, 2, 3, 8 anchors;
1, 3, 5, 20 classes; T of 1, 3, 50; one head whose two strides differ.

TARGETS: found by a directed search on the CPU (`threshold_targets`), in the reference's own fp32 arithmetic (`iou32`, which
test_cpu_loss_cases.py holds to oracle/loss_oracle.py::_bbox_iou bit for bit): boxes whose IoU with an anchor is EXACTLY the ignore
threshold, one fp32 step below and one above it, and among the exact ones those whose decision flips when the compiler contracts the
union `b1 + b2 - inter` into FMAs (`iou32(..., contracted=True)`: fma(a, b, c) = float32(float64(a) * float64(b) + float64(c)), the
product of two float32 being exact in float64).  Then the ties and collisions of get_target's sequential loop, the cell-index edges, and
the targets the reference cannot index.

  x * fw cannot round UP to fw for x < 1.  Let 2^e <= fw < 2^(e+1); float32 values just below fw are 2^(e-23) apart, and
  fw - x * fw = fw * (1 - x) >= fw * 2^-24 >= 2^(e-24), half that spacing, with equality only for fw = 2^e, where the product is
  exact.  So the largest float32 below 1 always lands in the last column and only x >= 1 is outside the map; the table has both.  The
  rounding that does exist is across an INTERIOR boundary: x < k / fw with float32(x * fw) == k, on a 20-column map (`roundup`).

LOGITS: set M is N(0, 3) clipped to +-12.  Set S puts values of {+-20, +-30, +-60, +-80, +-110, +-1000} on about half of all entries,
positive, no-object and ignored cells alike (the rest is M).  Two bands are deliberately NOT in S:
  (15, 18)     float32 sigmoid is within a few ulps of 1 without being 1: one ulp of difference in expf turns log(1 - p) from about
               -16.6 into the clamp -100, so neither fp32 implementation is "right" there and no float64 model can referee;
  (-105, -86)  p is a float32 subnormal: 1 / (1 + expf(-x)) flushes or not depending on the division's denormal mode.
Two band-only cases draw from these bands and assert nothing but "every loss and gradient finite, or the documented NaN".

THE COMPARATOR (`judge`), the same for the CPU and GPU files; m64 = oracle/loss_oracle.py::loss_model64, twin = loss_head in float32
with torch autograd (the reference's own arithmetic):
  planes   mask, noobj, tx, ty, every class plane: bit for bit get_target.  tw, th: within one float32 ulp (the device's double log and
           the host's may round differently); the number of non-identical values is reported (expected 0).
  [7]      the count of targets the reference cannot index: exact.
  losses   each of the seven: |dev - m64| <= max(3 |twin - m64|, 8 float32 ulps of |m64|); NaN exactly where the model has NaN.
           3 = ACCURACY_RATIO of test_gpu_io_params.py; 8 ulps = loss_final_kernel's ten fp32 operations on top of the store.
  grad     per kind (x, y, w, h, conf_pos, conf_noobj, cls) over the cells of that kind:
           max|dev - m64| <= max(3 max|twin - m64|, 4 float32 ulps of the kind's max|m64|);
           a kind whose model gradient is identically zero (always: box_off, conf_ignored, cls_off) must be exactly zero.
No bound comes from what the device computes.  `twin_condition` is what the table itself must satisfy: the twin within the ulp floors
alone (8 ulps per loss, 4 ulps of the kind's maximum per gradient element) plus what SIGMOID_ULPS = 2 float32 steps of every sigmoid are
worth.  The allowance is needed because the model's sigmoid is correctly rounded and torch's float32 one is up to 2 steps off (measured
on the CPU, asserted in test_cpu_loss_cases.py): at a logit of 10, one step of p moves log(1 - p) by 1e-3, far beyond 8 ulps of the
loss, already inside set M.  A logit value that broke this condition would leave the table; none had to.
"""
import collections
import math

import numpy as np
import torch

from oracle import loss_oracle as lo

F32 = np.float32
THRES = 0.5
ACCURACY_RATIO = 3.0
LOSS_ULPS, GRAD_ULPS = 8, 4
SIGMOID_ULPS = 2            # torch's float32 sigmoid on the CPU against float32(sigmoid64): test_cpu_loss_cases.py measures at most 2 steps
S_VALUES = np.array([20, 30, 60, 80, 110, 1000, -20, -30, -60, -80, -110, -1000], np.float32)
ANC_LARGE = [[10, 13], [16, 30], [33, 23]]          # the shipped 320x256 model's stride-16 head
ANC_SMALL = [[150, 75], [100, 100], [75, 150]]
ANC_8 = [[6, 8], [10, 13], [16, 30], [33, 23], [30, 61], [62, 45], [59, 119], [116, 90]]

Case = collections.namedtuple("Case", "name N A C fh fw H W T anchors targets logits why logit_set counted")


# ---- the reference's fp32 arithmetic in numpy (held to the oracle bit for bit by the CPU file) ----

def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def iou32(gw, gh, aw, ah, contracted=False):
    """general.py:29-52 for boxes [0, 0, gw, gh] and [0, 0, aw, ah], one float32 operation at a time.  contracted: the union
    b1 + b2 - inter as fma(-iw, ih, fma(gw + 1, gh + 1, b2)), what -ffp-contract=fast may make of it."""
    gw, gh, aw, ah = (np.asarray(v, np.float32) for v in (gw, gh, aw, ah))
    one, zero = F32(1), F32(0)
    iw, ih = np.maximum(np.minimum(gw, aw) - zero + one, zero), np.maximum(np.minimum(gh, ah) - zero + one, zero)
    inter = iw * ih
    b2 = (aw - zero + one) * (ah - zero + one)
    if contracted:
        union = _fma(-iw, ih, _fma(gw - zero + one, gh - zero + one, b2)) + F32(1e-16)
    else:
        union = (gw - zero + one) * (gh - zero + one) + b2 - inter + F32(1e-16)
    return inter / union


def anchors32(case):
    """the head's anchors in feature-map units as float32 [A, 2] (yolo_loss.py:52-56; torch stores the Python doubles as float32)"""
    return np.array(lo.scaled_anchors(case.anchors, (case.H, case.W), case.fh, case.fw), np.float64).astype(np.float32)


DEFECTS_TARGET = ("argmax_last", "thres_ge", "iou_contracted", "onehot_overwrites", "tx_first")


def get_target_np(target, anc, in_w, in_h, C, defect=None, thres=THRES):
    """get_target (yolo_loss.py:144-196) in numpy float32; defect=None is bit for bit oracle/loss_oracle.py::get_target.  target float32
    [N, T, 6] without targets the reference cannot index; anc float32 [A, 2].  -> (mask, noobj, tx, ty, tw, th [N, A, h, w], tcls [.., C])."""
    target = np.asarray(target, np.float32)
    N, A = target.shape[0], len(anc)
    mask, noobj = np.zeros((N, A, in_h, in_w), np.float32), np.ones((N, A, in_h, in_w), np.float32)
    tx, ty, tw, th = (np.zeros((N, A, in_h, in_w), np.float32) for _ in range(4))
    tcls = np.zeros((N, A, in_h, in_w, C), np.float32)
    seen = set()
    for b in range(N):
        for t in range(target.shape[1]):
            if target[b, t, 5] < 1:
                break
            gx, gy = target[b, t, 0] * F32(in_w), target[b, t, 1] * F32(in_h)
            gw, gh = target[b, t, 2] * F32(in_w), target[b, t, 3] * F32(in_h)
            if gw <= 0 or gh <= 0:
                continue
            gi, gj = int(gx), int(gy)
            iou = iou32(gw, gh, anc[:, 0], anc[:, 1], contracted=defect == "iou_contracted")
            noobj[b, (iou >= thres) if defect == "thres_ge" else (iou > thres), gj, gi] = 0
            best = int(np.argmax(iou)) if defect != "argmax_last" else A - 1 - int(np.argmax(iou[::-1]))
            mask[b, best, gj, gi] = 1
            if not (defect == "tx_first" and (b, best, gj, gi) in seen):
                tx[b, best, gj, gi] = gx - F32(gi)
            seen.add((b, best, gj, gi))
            ty[b, best, gj, gi] = gy - F32(gj)
            tw[b, best, gj, gi] = math.log(float(gw / anc[best, 0] + F32(1e-16)))
            th[b, best, gj, gi] = math.log(float(gh / anc[best, 1] + F32(1e-16)))
            if defect == "onehot_overwrites":
                tcls[b, best, gj, gi, :] = 0
            tcls[b, best, gj, gi, int(target[b, t, 4])] = 1
    return tuple(torch.from_numpy(a) for a in (mask, noobj, tx, ty, tw, th, tcls))


# ---- the directed search for boxes on the ignore threshold ----

def threshold_targets(anc, fh, fw, want=48, thres=THRES):
    """-> {"exact": [...], "below": [...], "above": [...]} of (w, h, anchor, flips): normalised float32 sizes whose fp32 IoU with `anchor`
    is exactly thres / the float32 just below / just above; flips: the decision iou > thres differs under the contracted union.  Directed:
    IoU = 1/2 means union = 2 inter, i.e. (box inside the anchor) area_anchor = 2 area_box or (anchor inside the box) the reverse; walk
    the width, solve for the height in float64, try the float32 heights around it.  At most `want` per set, flipping ones first."""
    t32 = F32(thres)
    lo32, hi32 = np.nextafter(t32, F32(0)), np.nextafter(t32, F32(1))
    found = {"exact": [], "below": [], "above": []}
    for a, (aw, ah) in enumerate(anc):
        b2 = (float(aw) + 1) * (float(ah) + 1)
        for inside in (True, False):
            wn = (np.linspace(0.05 * aw, aw, 600) if inside else np.linspace(aw, min(4 * aw + 2, 0.95 * fw), 600)) / fw
            wn = wn.astype(np.float32)
            gw = wn * F32(fw)
            gh64 = (b2 / 2 if inside else 2 * b2) / (gw.astype(np.float64) + 1) - 1
            ok = (gh64 > 0.02) & ((gh64 <= ah) if inside else ((gh64 >= ah) & (gh64 <= 0.95 * fh))) & ((gw <= aw) if inside else (gw >= aw))
            hn = (gh64[ok] / fh).astype(np.float32)
            for step in range(-6, 7):
                h = hn.copy()
                for _ in range(abs(step)):
                    h = np.nextafter(h, F32(2 if step > 0 else -1))
                w = wn[ok]
                v = iou32(w * F32(fw), h * F32(fh), aw, ah)
                vc = iou32(w * F32(fw), h * F32(fh), aw, ah, contracted=True)
                for key, val in (("exact", t32), ("below", lo32), ("above", hi32)):
                    for i in np.nonzero(v == val)[0]:
                        found[key].append((float(w[i]), float(h[i]), a, bool((v[i] > t32) != (vc[i] > t32))))
    out = {}
    for key, rows in found.items():
        rows = sorted(set(rows))
        pick = [r for r in rows if r[3]][:want // 2]        # those that flip under contraction first, then the anchors in turn
        rest = [[r for r in rows if not r[3] and r[2] == a] for a in range(len(anc))]
        for i in range(max(len(r) for r in rest)):
            pick += [r[i] for r in rest if i < len(r)]
        out[key] = pick[:want]
    return out


# ---- builders ----

def _empty(N, T):
    return np.zeros((N, T, 6), np.float32)


def _random_targets(rng, N, T, C, fill=None):
    """`fill` (default T) rows per image, the rest zero: the marker < 1 of the first zero row ends the list"""
    t = _empty(N, T)
    k = T if fill is None else fill
    t[:, :k, 0:2] = rng.uniform(0.02, 0.98, (N, k, 2))
    t[:, :k, 2:4] = rng.uniform(0.02, 0.9, (N, k, 2))
    t[:, :k, 4] = rng.integers(0, C, (N, k))
    t[:, :k, 5] = 255.0
    return t


def _logits(rng, N, A, C, fh, fw, kind):
    shape = (N, A * (5 + C), fh, fw)
    x = np.clip(rng.normal(0, 3, shape), -12, 12).astype(np.float32)
    if kind == "S":
        pick = rng.random(shape) < 0.5
        x[pick] = rng.choice(S_VALUES, int(pick.sum()))
    elif kind == "band":
        pick = rng.random(shape) < 0.5
        x[pick] = rng.uniform(15.0, 18.0, int(pick.sum())).astype(np.float32)
        x[~pick] = rng.uniform(-105.0, -86.0, int((~pick).sum())).astype(np.float32)
    return x


def _count(t, fh, fw, C):
    return lo.drop_unindexable(torch.from_numpy(t), fw, fh, C)[1]


def _case(name, seed, N, A, C, fh, fw, H, W, T, anchors, targets, why, logit_set="M"):
    assert targets.shape == (N, T, 6) and len(anchors) == A
    rng = np.random.default_rng(seed)
    return Case(name, N, A, C, fh, fw, H, W, T, anchors, np.ascontiguousarray(targets, np.float32), _logits(rng, N, A, C, fh, fw, logit_set),
                why, logit_set, _count(targets, fh, fw, C))


def _cell_xy(gi, gj, fw, fh, off=0.5):
    return (gi + off) / fw, (gj + off) / fh


def _threshold_case():
    fh, fw, H, W = 16, 20, 256, 320
    anc = np.array(lo.scaled_anchors(ANC_LARGE, (H, W), fh, fw), np.float64).astype(np.float32)
    sets = threshold_targets(anc, fh, fw)
    rows = [(k,) + r for k in ("exact", "below", "above") for r in sets[k]]
    T = 50
    N = -(-len(rows) // T)
    t = _empty(N, T)
    for i, (k, w, h, a, flips) in enumerate(rows):          # one cell each, so that no target hides another's ignore marks
        n, j = divmod(i, T)
        x, y = _cell_xy(j % fw, (j // fw) * 5 + 1, fw, fh)
        t[n, j] = (x, y, w, h, i % 3, 255.0)
    return t, rows, (N, 3, 3, fh, fw, H, W, T)


def build_cases():
    rng = np.random.default_rng(20240611)
    cases = []

    def add(name, N, A, C, fh, fw, H, W, T, anchors, targets, why, logit_set="M"):
        cases.append(_case(name, len(cases) + 1, N, A, C, fh, fw, H, W, T, anchors, targets, why, logit_set))

    # geometry
    add("e3", 1, 3, 3, 1, 1, 16, 16, 1, ANC_LARGE, _random_targets(rng, 1, 1, 3), "E = 3 < 16 accumulators; 1x1 map; T = 1")
    add("e15", 1, 1, 1, 3, 5, 48, 80, 3, [[16, 30]], _random_targets(rng, 1, 3, 1), "E = 15; one anchor, one class; odd 3x5 map")
    add("e16", 2, 8, 3, 1, 1, 32, 32, 1, ANC_8, _random_targets(rng, 2, 1, 3), "E = 16; 8 anchors")
    add("e17", 1, 1, 5, 1, 17, 16, 272, 3, [[16, 30]], _random_targets(rng, 1, 3, 5), "E = 17; 5 classes")
    add("e255", 1, 1, 3, 15, 17, 240, 272, 50, [[33, 23]], _random_targets(rng, 1, 50, 3), "E = 255: one ragged workgroup; T = 50 all used")
    add("e256", 1, 1, 20, 16, 16, 256, 256, 3, [[33, 23]], _random_targets(rng, 1, 3, 20), "E = 256: exactly one workgroup; 20 classes")
    add("e257", 1, 1, 3, 1, 257, 16, 4112, 50, [[16, 30]], _random_targets(rng, 1, 50, 3, 20), "E = 257: a second workgroup of one cell")
    t = _random_targets(rng, 64, 3, 3)
    t[5] = 0; t[63] = 0                                   # empty images among full ones
    t[7, 0, 5] = 0                                        # an end marker in row 0 in front of two valid rows
    t[9, 1, 5] = 0.5                                      # a marker < 1 that is not 0
    add("n64", 64, 2, 3, 4, 6, 64, 96, 3, ANC_LARGE[:2], t, "N = 64: one full workgroup of loss_targets_kernel; 2 anchors; empty images, end marker in row 0")
    add("n65", 65, 3, 1, 3, 5, 48, 80, 3, ANC_LARGE, _random_targets(rng, 65, 3, 1, 2), "N = 65: a second workgroup with one image; 1 class")
    t = _random_targets(rng, 130, 3, 3)
    t[64] = 0; t[129, 1:] = 0
    add("n130", 130, 3, 3, 4, 6, 128, 192, 3, ANC_SMALL, t, "N = 130: three workgroups, the last with two images")
    add("large", 2, 3, 3, 16, 20, 256, 320, 50, ANC_LARGE, _random_targets(rng, 2, 50, 3, 37), "the shipped stride-16 head, T = 50 padded after 37")
    add("small", 3, 3, 5, 8, 10, 256, 320, 50, ANC_SMALL, _random_targets(rng, 3, 50, 5), "the shipped stride-32 head with 5 classes, T = 50 all used")
    add("strides", 2, 3, 3, 4, 6, 128, 96, 3, ANC_LARGE, _random_targets(rng, 2, 3, 3), "H / fh = 32 but W / fw = 16")
    add("a8c20", 2, 8, 20, 3, 5, 96, 160, 50, ANC_8, _random_targets(rng, 2, 50, 20, 30), "8 anchors x 20 classes on the odd map")
    t = _empty(3, 3)
    t[:, :, :5] = _random_targets(rng, 3, 3, 3)[:, :, :5]   # plausible rows, every marker 0: an all-noCloud batch
    add("nopos", 3, 3, 3, 4, 6, 64, 96, 3, ANC_LARGE, t, "no target at all: NaN class loss and total, the gradient still defined")

    # the ignore threshold
    t, rows, (N, A, C, fh, fw, H, W, T) = _threshold_case()
    add("thres", N, A, C, fh, fw, H, W, T, ANC_LARGE, t, "IoU exactly on, one float32 below and one above ignore_thres; %d rows" % len(rows))

    # best-anchor ties
    t = _random_targets(rng, 2, 8, 3)
    add("tie_same", 2, 3, 3, 4, 6, 64, 96, 8, [[20, 20], [20, 20], [6, 8]], t, "two identical anchors: the first maximum wins")
    t = _random_targets(rng, 2, 8, 3)
    t[:, :, 3] = t[:, :, 2]                               # square targets, equal strides: IoU with (a, b) and (b, a) is the same float32
    add("tie_swap", 2, 3, 3, 16, 16, 256, 256, 8, [[16, 30], [30, 16], [10, 13]], t, "anchors (a, b) / (b, a), square targets, equal strides")

    # several targets in one cell
    t = _empty(2, 8)
    for n in range(2):
        for k in range(4):                                # cell (2, 1): same size -> same best anchor; classes 0, 1, 2, 0; tx from the last
            t[n, k] = ((2 + 0.1 + 0.2 * k) / 6, (1 + 0.8 - 0.15 * k) / 4, 0.30, 0.45, k % 3, 255.0)
        t[n, 4] = (0.9, 0.9, 0.2, 0.2, 1, 255.0)
    add("cell_same", 2, 3, 3, 4, 6, 64, 96, 8, ANC_LARGE, t, "four targets in one cell with one best anchor: the one-hot accumulates, tx..th are the last one's")
    t = _empty(1, 8)
    for k, (w, h) in enumerate(((10 / 96, 13 / 64), (16 / 96, 30 / 64), (33 / 96, 23 / 64), (16 / 96, 30 / 64))):
        t[0, k] = (3.4 / 6, 2.6 / 4, w, h, k % 3, 255.0)  # cell (3, 2): each anchor in turn is the best one
    add("cell_diff", 1, 3, 3, 4, 6, 64, 96, 8, ANC_LARGE, t, "four targets in one cell with three different best anchors")

    # cell-index edges
    t = _empty(2, 24)
    k = 0
    for gi in (0, 1, 7, 15):                              # gx, gy exactly integral (fw = fh = 16: the products are exact)
        t[0, k] = (gi / 16, ((gi * 5) % 16) / 16, 0.2, 0.3, k % 3, 255.0); k += 1
    for e in (1, 2, 5, 10, 15, 19):                       # gx = fw - 2^-e, gy = fh - 2^-e: the last column and row
        t[0, k] = ((16 - 2.0 ** -e) / 16, (16 - 2.0 ** -(e + 1)) / 16, 0.1, 0.1, k % 3, 255.0); k += 1
    t[1, 0] = (float(np.nextafter(F32(1), F32(0))), float(np.nextafter(F32(1), F32(0))), 0.1, 0.2, 1, 255.0)
    add("edges", 2, 3, 3, 16, 16, 256, 256, 24, ANC_LARGE, t, "gx, gy exactly integral, at fw - 2^-k, and the largest float32 below 1")
    t = _empty(1, 8)
    ks = interior_roundups(20)
    assert len(ks) >= 3
    for k, (xn, col) in enumerate(ks[:6]):
        t[0, k] = (xn, (k + 0.5) / 16, 0.1, 0.1, k % 3, 255.0)
    t[0, 6] = (float(np.nextafter(F32(1), F32(0))), 0.5, 0.1, 0.1, 0, 255.0)
    add("roundup", 1, 3, 3, 16, 20, 256, 320, 8, ANC_LARGE, t, "x < k / fw whose float32 product IS k: the target belongs to column k")

    # skipped targets
    t = _empty(2, 8)
    t[0, 0] = (0.30, 0.30, 0.0, 0.2, 0, 255.0)            # zero width
    t[0, 1] = (0.30, 0.30, -0.1, 0.2, 1, 255.0)           # negative width
    t[0, 2] = (0.30, 0.30, 0.2, -0.0, 1, 255.0)           # minus zero height
    t[0, 3] = (0.30, 0.30, 0.2, 0.3, 2, 255.0)            # the same cell: lands
    t[1, 0] = (0.5, 0.5, 0.2, 0.0, 0, 255.0)
    add("skipped", 2, 3, 3, 4, 6, 64, 96, 8, ANC_LARGE, t, "zero / negative sizes are skipped and a later target of the same cell still lands")

    # class ids
    t = _empty(1, 8)
    t[0, 0] = (0.2, 0.2, 0.2, 0.3, 2.7, 255.0)            # int() truncates: class 2
    t[0, 1] = (0.6, 0.6, 0.2, 0.3, 0.9, 255.0)            # class 0
    add("cls_trunc", 1, 3, 3, 4, 6, 64, 96, 8, ANC_LARGE, t, "class ids 2.7 and 0.9 truncate to 2 and 0")

    # targets the reference cannot index: counted in losses[7], skipped whole
    t = _empty(3, 4)
    t[0, 0] = (0.2, 0.2, 0.2, 0.3, 3, 255.0)              # class == C
    t[0, 1] = (0.7, 0.7, 0.2, 0.3, 1, 255.0)
    t[1, 0] = (0.2, 0.2, 0.2, 0.3, -1, 255.0)             # class -1 (the reference wraps round to the last class)
    t[1, 1] = (0.2, 0.2, 0.3, 0.3, 1, 255.0)              # the same cell, valid
    t[2, 0] = (-1.5 / 6, 0.5, 0.2, 0.3, 0, 255.0)         # column index -1 (the reference wraps round to the last column)
    t[2, 1] = (1.0, 0.5, 0.2, 0.3, 0, 255.0)              # x == 1: column index == fw
    t[2, 2] = (0.5, 1.25, 0.2, 0.3, 0, 255.0)             # row index == fh + 1
    t[2, 3] = (0.5, 0.5, 0.2, 0.3, 2, 255.0)
    add("counted", 3, 3, 3, 4, 6, 64, 96, 4, ANC_LARGE, t, "class C, class -1, column -1, column fw, row fh + 1: five counted, three land")

    # set S and the bands
    by = {c.name: c for c in cases}
    for name in ("e3", "n65", "small", "thres", "nopos", "cell_same", "a8c20"):
        c = by[name]
        add(name + "_S", c.N, c.A, c.C, c.fh, c.fw, c.H, c.W, c.T, c.anchors, c.targets, c.why + "; logits of set S", "S")
    for name in ("small", "nopos"):
        c = by[name]
        add(name + "_band", c.N, c.A, c.C, c.fh, c.fw, c.H, c.W, c.T, c.anchors, c.targets, c.why + "; logits of the two excluded bands", "band")
    return cases, rows


def interior_roundups(fw):
    """[(x, k)]: float32 x with x < k / fw in exact arithmetic and float32(x * fw) == k, 0 < k < fw"""
    out = []
    for k in range(1, fw):
        x = F32(k / fw)
        for _ in range(3):
            if float(x) * fw < k and x * F32(fw) == F32(k):
                out.append((float(x), k))
                break
            x = np.nextafter(x, F32(0))
    return out


_built = {}


def cases():
    if not _built:
        _built["cases"], _built["thres_rows"] = build_cases()
    return _built["cases"]


def threshold_rows():
    cases()
    return _built["thres_rows"]


def case_by_name(name):
    return {c.name: c for c in cases()}[name]


# ---- the reference of a case, computed once and left unchanged ----

_refs = {}


def reference(case):
    """-> dict: planes (get_target on the indexable targets), counted, m64 (loss_model64's dict), twin_losses float32 [7], twin_grad float32,
    kinds.  Cached per case name."""
    if case.name not in _refs:
        t = torch.from_numpy(case.targets)
        clean, counted = lo.drop_unindexable(t, case.fw, case.fh, case.C)
        x = torch.from_numpy(case.logits)
        planes = lo.get_target(clean, lo.scaled_anchors(case.anchors, (case.H, case.W), case.fh, case.fw), case.fw, case.fh, THRES, case.C)
        m64 = lo.loss_model64(x, clean, case.anchors, case.C, (case.H, case.W), THRES, planes=planes)
        tl, tg = lo.loss_and_grad(x, clean, case.anchors, case.C, (case.H, case.W), THRES)
        _refs[case.name] = dict(planes=planes, counted=counted, clean=clean, m64=m64, twin_losses=tl, twin_grad=tg.numpy(),
                                kinds=lo.grad_kinds(planes, case.C))
    return _refs[case.name]


def planes_to_dense(planes):
    """the seven planes of get_target -> float32 [6 + C, E], the layout behind the workspace's 16 doubles"""
    flat = [p.numpy().reshape(-1) for p in planes[:6]]
    tc = planes[6].numpy()
    return np.stack(flat + [tc[..., k].reshape(-1) for k in range(tc.shape[-1])]).astype(np.float32)


# ---- the comparator ----

def ulp32(v):
    return float(np.spacing(np.float32(abs(v))))


class Report:
    def __init__(self, case):
        self.case, self.rows, self.failures, self.plane_diffs = case, [], [], 0

    @property
    def ok(self):
        return not self.failures

    def add(self, what, dev, twin, bound, ok):
        self.rows.append((what, dev, twin, bound))
        if not ok:
            self.failures.append("%s %s: device %.3e, twin %.3e, bound %.3e" % (self.case.name, what, dev, twin, bound))

    def table(self):
        head = "[loss %s] N=%d A=%d C=%d %dx%d T=%d set %s: tw/th values not identical %d" % (
            self.case.name, self.case.N, self.case.A, self.case.C, self.case.fh, self.case.fw, self.case.T, self.case.logit_set, self.plane_diffs)
        return head + "\n" + "\n".join("  %-14s device %.3e  twin %.3e  bound %.3e" % r for r in self.rows)


def judge_planes(rep, dense, ref_planes):
    want = planes_to_dense(ref_planes)
    if dense.shape != want.shape:
        rep.failures.append("%s planes: shape %s, want %s" % (rep.case.name, dense.shape, want.shape))
        return
    names = ["mask", "noobj", "tx", "ty", "tw", "th"] + ["class%d" % k for k in range(want.shape[0] - 6)]
    for p, name in enumerate(names):
        a, b = dense[p], want[p]
        if name in ("tw", "th"):
            rep.plane_diffs += int((a.view(np.int32) != b.view(np.int32)).sum())
            bad = ~(np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.abs(b)).astype(np.float64))
        else:
            bad = a.view(np.int32) != b.view(np.int32)
        if bad.any():
            i = int(np.nonzero(bad)[0][0])
            rep.failures.append("%s plane %s: %d of %d values differ, first at %d: %r, want %r" % (rep.case.name, name, int(bad.sum()), a.size, i, a[i], b[i]))


def judge_losses(rep, losses, m64, twin):
    for i, name in enumerate(lo.LOSS_NAMES):
        d, w, t = float(losses[i]), float(m64[i]), float(twin[i])
        if math.isnan(w):
            rep.add("loss " + name, float("nan"), float("nan"), float("nan"), math.isnan(d))
            continue
        bound = max(ACCURACY_RATIO * abs(t - w), LOSS_ULPS * ulp32(w))
        rep.add("loss " + name, abs(d - w), abs(t - w), bound, math.isfinite(d) and abs(d - w) <= bound)


def judge_grad(rep, grad, m64, twin, kinds):
    grad = np.asarray(grad, np.float64).reshape(next(iter(kinds.values())).shape)
    m64, twin = m64.reshape(grad.shape), np.asarray(twin, np.float64).reshape(grad.shape)
    for name in lo.GRAD_KINDS:
        sel = kinds[name]
        if not sel.any():
            continue
        g, w, t = grad[sel], m64[sel], twin[sel]
        top = np.abs(w).max()
        if top == 0:
            rep.add("grad " + name, float(np.abs(np.nan_to_num(g, nan=np.inf)).max()), float(np.abs(t).max()), 0.0, bool((g == 0).all()))
            continue
        d, dt = np.abs(g - w).max(), np.abs(t - w).max()
        bound = max(ACCURACY_RATIO * dt, GRAD_ULPS * ulp32(top))
        rep.add("grad " + name, float(d), float(dt), bound, bool(np.isfinite(g).all() and d <= bound))


def judge(case, losses8, grad=None, dense=None, ref=None):
    """losses8: the eight float32 of d_losses; grad: like the logits or None; dense: float32 [6 + C, E] or None -> Report"""
    ref = ref or reference(case)
    rep = Report(case)
    if dense is not None:
        judge_planes(rep, dense, ref["planes"])
    if float(losses8[7]) != float(ref["counted"]):
        rep.failures.append("%s losses[7] = %r, want %d" % (case.name, float(losses8[7]), ref["counted"]))
    if case.logit_set == "band":
        want_nan = ref["m64"]["n_pos"] == 0
        fin = [math.isfinite(float(v)) for v in losses8[:7]]
        ok = all(fin[1:6]) and (fin[0] and fin[6]) != want_nan and (grad is None or bool(np.isfinite(grad).all()))
        if not ok:
            rep.failures.append("%s: a loss or gradient of the band case is not finite (or not the documented NaN): %r" % (case.name, list(losses8)))
        return rep
    judge_losses(rep, losses8, ref["m64"]["losses"], ref["twin_losses"])
    if grad is not None:
        judge_grad(rep, grad, ref["m64"]["grad"], ref["twin_grad"], ref["kinds"])
    return rep


def twin_condition(case):
    """[failures]: what the table itself must satisfy.  The twin against the model within the ulp floors alone (LOSS_ULPS per loss, GRAD_ULPS
    of the kind's maximum per gradient element) plus what SIGMOID_ULPS float32 steps of every sigmoid are worth (loss_model64's p_ulp_*):
    the model's sigmoid is correctly rounded, torch's float32 one is not, and at |logit| near 12 one step of p moves log(1 - p) by 1e-2."""
    ref = reference(case)
    m = ref["m64"]
    out = []
    for i, name in enumerate(lo.LOSS_NAMES):
        w, t = float(m["losses"][i]), float(ref["twin_losses"][i])
        bound = LOSS_ULPS * ulp32(w) + SIGMOID_ULPS * float(m["p_ulp_losses"][i]) if not math.isnan(w) else 0.0
        if math.isnan(w) != math.isnan(t) or (not math.isnan(w) and abs(t - w) > bound):
            out.append("%s loss %s: twin %r, model %r, off by %.3e, allowed %.3e" % (case.name, name, t, w, abs(t - w), bound))
    shape = next(iter(ref["kinds"].values())).shape
    g, w, dg = (a.astype(np.float64).reshape(shape) for a in (ref["twin_grad"], m["grad"], m["p_ulp_grad"]))
    for name in lo.GRAD_KINDS:
        sel = ref["kinds"][name]
        if not sel.any():
            continue
        a, b = g[sel], w[sel]
        top = np.abs(b).max()
        over = np.abs(a - b) - (GRAD_ULPS * ulp32(top) + SIGMOID_ULPS * dg[sel]) if top > 0 else np.abs(a)
        if over.max() > 0:
            out.append("%s grad %s: twin off by %.3e beyond what is allowed (kind's maximum %.3e)" % (case.name, name, over.max(), top))
    return out
