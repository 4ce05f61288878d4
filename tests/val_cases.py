"""Case generators for the validation-time NMS and decode (`val_nms_kernel`, `val_decode_kernel`): synthetic prediction tensors that reach
what trained-network goldens never do -- every pad size up to the 8191-row limit, compaction trips in which all / no rows pass, pass counts
around the powers of two of the bitonic pad, tied confidences, tied class scores, thresholds hit exactly, zero-size / huge / infinite boxes,
ragged batches, more survivors than `kmax`.  Shared by tests/test_cpu_val_cases.py (the oracle alone: every case does what it names) and
tests/test_gpu_val_nms.py (the kernels against the oracle).  Everything is deterministic (numpy-seeded).

A case is a `Case`: `pred` float32 [N, M, 5 + C] in centre format (cx, cy, w, h, conf, cls...), the two thresholds, and what the case
claims: `K` (rows at or above `conf_thres`, per frame) and a few flags.  `reference(case)` runs oracle/val_oracle.py::non_max_suppression
on it once and keeps the result."""
import numpy as np
import torch

POST_THREADS = 1024          # rows per trip of val_nms_kernel's compaction loop (csrc/yf_post_kernels.hip)
CANVAS_W, CANVAS_H = 640, 512
SIZE_LADDER_M = (1, 63, 64, 65, 255, 256, 257, 1200, 4096, 4097, 4800, 8191)
PASS_LADDER_K = (0, 1, 64, 65, 256, 257, 1024, 1025, None)      # None: K = M
PLACEMENTS = ("scattered", "first_trip", "last_trip")
TIE_VALUES = np.array([0.3, 0.45, 0.5, 0.55, 0.7, 0.8, 0.95], np.float32)    # 0.5 is the threshold itself: it passes
F32 = np.float32


class Case:
    def __init__(self, name, pred, conf_thres, nms_thres, K=None, **flags):
        self.name = name
        self.pred = torch.from_numpy(np.ascontiguousarray(pred, dtype=np.float32))
        self.C = self.pred.shape[2] - 5
        self.conf_thres, self.nms_thres = conf_thres, nms_thres
        self.K = K                        # intended rows at or above conf_thres, one per frame (None: not forced)
        self.flags = flags

    def __repr__(self):
        return "Case(%s, %s)" % (self.name, tuple(self.pred.shape))


def _boxes(rng, shape, C, lo=20.0, hi=240.0):
    """random boxes in the canvas, uniform confidences (about half pass 0.5), uniform class scores"""
    p = np.empty(shape + (5 + C,), np.float32)
    p[..., 0] = rng.uniform(0, CANVAS_W, shape)
    p[..., 1] = rng.uniform(0, CANVAS_H, shape)
    p[..., 2] = rng.uniform(lo, hi, shape)
    p[..., 3] = rng.uniform(lo, hi, shape)
    p[..., 4] = rng.uniform(0, 1, shape)
    p[..., 5:] = rng.uniform(0, 1, shape + (C,))
    return p


def _force_pass(rng, conf, rows, thres=0.5):
    """conf[rows] in [thres, 1), every other row in [0, thres): exactly len(rows) rows pass"""
    t = F32(thres)
    conf[:] = rng.uniform(0, 1, conf.shape).astype(np.float32) * np.nextafter(t, F32(0))     # < thres in fp32
    hi = (t + rng.uniform(0, 1, len(rows)) * (1 - thres)).astype(np.float32)
    conf[rows] = np.minimum(np.maximum(hi, t), np.nextafter(F32(1), F32(0)))
    assert int((conf >= t).sum()) == len(rows)


def size_ladder():
    """every pad size of launch_val_nms (64 .. 8192 rows, the 48 KiB LDS step between M = 4096 and 4097, the 8191-row limit), M around the
    64-lane wave and the 1024-row trip.  M = 1 cannot suppress anything: frame 0 passes, frame 1 does not."""
    out = []
    for M in SIZE_LADDER_M:
        rng = np.random.default_rng(1000 + M)
        p = _boxes(rng, (2, M), 3)
        if M == 1:
            p[0, 0, 4], p[1, 0, 4] = 0.9, 0.1
        out.append(Case("size_M%d" % M, p, 0.5, 0.2, degenerate=(M == 1)))
    return out


def _placed_rows(rng, M, K, placement):
    if placement == "scattered":
        return np.sort(rng.choice(M, K, replace=False))
    if placement == "first_trip":             # rows 0 .. K-1: the first trip passes whole (K >= 1024), every later one not at all
        return np.arange(K)
    return np.arange(M - K, M)                # the last (partial) trip first, growing backwards


def pass_ladder():
    """exactly K rows at or above the threshold, K around the powers of two the sort pads to, one frame per K; the passing rows scattered,
    packed from row 0, or packed from the last row back (trips of the compaction loop in which every / no row passes)."""
    out = []
    for M in (1200, 4800):
        for pl in PLACEMENTS:
            rng = np.random.default_rng(2000 + M + PLACEMENTS.index(pl))
            Ks = [M if k is None else k for k in PASS_LADDER_K]
            p = _boxes(rng, (len(Ks), M), 3)
            for f, K in enumerate(Ks):
                _force_pass(rng, p[f, :, 4], _placed_rows(rng, M, K, pl))
            out.append(Case("pass_M%d_%s" % (M, pl), p, 0.5, 0.2, K=Ks, ladder=True))
    return out


def ties():
    """M = 600, confidences from 7 fp32 values only: equal keys but for the row index.  Rows 100 .. 199 and 300 .. 379 are runs of one value
    (longer than a wave), the classes are random, so every value occurs in every class and equal neighbours straddle class boundaries.
    `identical`: tied rows of one class also carry one and the same box."""
    out = []
    for identical in (False, True):
        rng = np.random.default_rng(3000 + identical)
        p = _boxes(rng, (2, 600), 3)
        idx = rng.integers(0, len(TIE_VALUES), (2, 600))
        idx[:, 100:200] = 4
        idx[:, 300:380] = 2
        p[..., 4] = TIE_VALUES[idx]
        if identical:
            table = _boxes(rng, (len(TIE_VALUES),), 3)[:, :4]
            p[..., :4] = table[idx]
        K = [int((p[f, :, 4] >= F32(0.5)).sum()) for f in range(2)]
        out.append(Case("ties_identical" if identical else "ties", p, 0.5, 0.2, K=K, ties=True))
    return out


def class_argmax():
    """C in {1, 2, 3, 20, 80}; for C >= 2, 10 % of the rows have two or more equal maximal class scores.  The expected class is what
    torch.max returns on the host that runs the oracle (the first maximum): the kernel's `v > best` scan is pinned to that."""
    out = []
    for C in (1, 2, 3, 20, 80):
        rng = np.random.default_rng(4000 + C)
        p = _boxes(rng, (2, 1200), C)
        ntied = 0
        if C >= 2:
            for f in range(2):
                rows = rng.choice(1200, 120, replace=False)
                for r in rows:
                    k = int(rng.integers(2, min(C, 4) + 1))
                    where = rng.choice(C, k, replace=False)
                    p[f, r, 5 + where] = F32(p[f, r, 5:].max()) if rng.integers(2) else F32(1.0)
                ntied += len(rows)
        out.append(Case("argmax_C%d" % C, p, 0.5, 0.2, tied_rows=ntied))
    return out


def conf_threshold_equality():
    """conf_thres 0.5 (exact in fp32), 0.7 and 0.3 (not): 10 rows each at np.float32(thres), the fp32 value below and the one above.  torch
    compares a float32 tensor with a Python float in float32, the kernel takes (float)thres: rows AT float32(thres) pass, although
    float32(0.7) < 0.7.  The 0.7 case also uses nms_thres = 0.7."""
    out = []
    for thres in (0.5, 0.7, 0.3):
        rng = np.random.default_rng(5000 + int(thres * 10))
        t = F32(thres)
        p = _boxes(rng, (2, 300), 3)
        far = np.abs(p[..., 4] - t) < 1e-3
        p[..., 4][far] = 0.9
        for f in range(2):
            rows = rng.choice(300, 30, replace=False)
            p[f, rows[:10], 4] = t
            p[f, rows[10:20], 4] = np.nextafter(t, F32(0))
            p[f, rows[20:], 4] = np.nextafter(t, F32(1))
        K = [int((p[f, :, 4] >= t).sum()) for f in range(2)]
        out.append(Case("conf_eq_%g" % thres, p, thres, 0.7 if thres == 0.7 else 0.2, K=K))
    return out


# (W1, H1, W2, H2) in pixels, +1 convention: box 2 lies inside box 1, both with their top-left corner at the pair's origin.  The first entry of
# each threshold is the exact one (W2 H2 / W1 H1 == thres); the others were found by search so that the ORACLE's fp32 arithmetic -- the
# products round, and so does a1 + a2 above 2^24 -- gives the fp32 value next below / next above the threshold.
IOU_PAIRS = {
    0.25: {"equal": (40, 10, 10, 10), "below": (3841, 3025, 982, 2958), "above": (2703, 2889, 718, 2719)},
    0.5: {"equal": (40, 10, 20, 10), "below": (2878, 3903, 1439, 3903), "above": (2283, 2781, 1496, 2122)},
}
IOU_PAIR_ORDER = ("equal", "below", "above")


def _corner_row(x1, y1, wpx, hpx, conf, C=3, cls=0):
    """integer-aligned box of wpx x hpx PIXELS (corners x1 .. x1 + wpx - 1) in centre format: every value exact in fp32"""
    r = np.zeros(5 + C, np.float32)
    r[0], r[1], r[2], r[3], r[4] = x1 + (wpx - 1) / 2.0, y1 + (hpx - 1) / 2.0, wpx - 1, hpx - 1, conf
    r[5 + cls] = 0.9
    return r


def iou_threshold_equality():
    """pairs of one class whose IoU is exactly nms_thres (dropped: the reference keeps `iou < thres`), the fp32 value below it (kept) and
    above it (dropped); the pairs are 10000 px apart, so each box meets only its partner.  8 pairs of every kind, in two frames."""
    out = []
    for thres, pairs in IOU_PAIRS.items():
        rows = [[], []]
        for f in range(2):
            n = 0
            for rep in range(4):
                for kind in IOU_PAIR_ORDER:
                    W1, H1, W2, H2 = pairs[kind]
                    ox, oy = 10000 * n, 10000 * (n % 3)
                    conf = 0.99 - 0.01 * n
                    rows[f].append(_corner_row(ox, oy, W1, H1, conf))
                    rows[f].append(_corner_row(ox, oy, W2, H2, conf - 0.3))
                    n += 1
            order = np.random.default_rng(5500 + f).permutation(len(rows[f]))
            rows[f] = [rows[f][i] for i in order]
        p = np.array(rows, np.float32)
        out.append(Case("iou_eq_%g" % thres, p, 0.5, thres, K=[p.shape[1]] * 2, survivors=[12 + 4] * 2))
    return out


def degenerate_boxes():
    """zero-size boxes (area 1 by the +1 convention), boxes of 1e6 px, and w / h = +inf as exp() of a diverged logit gives.  Frame 0: the
    infinite rows carry the highest confidences of their classes (they are kept first and meet every other row); frame 1: the lowest."""
    rng = np.random.default_rng(6000)
    C = 3
    p = _boxes(rng, (2, 400), C)
    p[..., 4] = rng.uniform(0.3, 0.95, (2, 400))
    inf = F32(np.inf)
    for f in range(2):
        rows = rng.choice(400, 72, replace=False)
        p[f, rows[0:8], 2] = 0
        p[f, rows[8:16], 3] = 0
        p[f, rows[16:24], 2:4] = 0
        p[f, rows[20:24], :2] = p[f, rows[16:20], :2]             # zero-size boxes at the same point: IoU 1
        p[f, rows[24:36], 2:4] = rng.uniform(0.5e6, 1e6, (12, 2))
        p[f, rows[36:48], 2] = inf
        p[f, rows[48:60], 3] = inf
        p[f, rows[60:72], 2:4] = inf
        infrows = rows[36:72]
        if f == 0:
            p[f, infrows, 4] = rng.uniform(0.96, 0.999, len(infrows))
        else:
            low = (p[f, :, 4] >= 0.5) & (p[f, :, 4] < 0.53)
            p[f, low, 4] = 0.4
            p[f, infrows, 4] = rng.uniform(0.5, 0.52, len(infrows))
    return [Case("degenerate", p, 0.5, 0.2, inf=True)]


def ragged_batch():
    rng = np.random.default_rng(7000)
    Ks = [900, 0, 1, 0, 1200]
    p = _boxes(rng, (5, 1200), 3)
    for f, K in enumerate(Ks):
        _force_pass(rng, p[f, :, 4], _placed_rows(rng, 1200, K, "scattered"))
    return [Case("ragged", p, 0.5, 0.2, K=Ks)]


OVERFLOW_KMAX = 64


def overflow():
    """more than OVERFLOW_KMAX survivors in frame 1 of 3 (small boxes, a high NMS threshold); frames 0 and 2 stay below it"""
    rng = np.random.default_rng(8000)
    p = _boxes(rng, (3, 1200), 3, lo=10.0, hi=60.0)
    for f, K in enumerate((30, 700, 0)):
        _force_pass(rng, p[f, :, 4], _placed_rows(rng, 1200, K, "scattered"))
    return [Case("overflow", p, 0.5, 0.6, K=[30, 700, 0], overflow=True)]


GROUPS = {
    "size_small": lambda: [c for c in size_ladder() if c.pred.shape[1] <= 1200],
    "size_large": lambda: [c for c in size_ladder() if c.pred.shape[1] > 1200],
    "pass_1200": lambda: [c for c in pass_ladder() if c.pred.shape[1] == 1200],
    "pass_4800": lambda: [c for c in pass_ladder() if c.pred.shape[1] == 4800],
    "ties": ties,
    "argmax": class_argmax,
    "thresholds": lambda: conf_threshold_equality() + iou_threshold_equality(),
    "degenerate": degenerate_boxes,
    "ragged": ragged_batch,
    "overflow": overflow,
}

_CASES, _REF = {}, {}


def cases(group):
    """the cases of one group, generated once"""
    if group not in _CASES:
        _CASES[group] = GROUPS[group]()
    return _CASES[group]


def reference(case):
    """oracle/val_oracle.py::non_max_suppression on the case, computed once and shared (callers must not modify it)"""
    from oracle import val_oracle as vo
    if case.name not in _REF:
        _REF[case.name] = vo.non_max_suppression(case.pred, case.C, case.conf_thres, case.nms_thres)
    return _REF[case.name]


# ---- decode inputs ---------------------------------------------------------------------------------------------------------------

PLANTED_LOGITS = np.array([0.0, -0.0, 1e-30, -1e-30, 20, -20, 87, -87, 88.7, 89, 100, -100, -104], np.float32)


def decode_head(seed, bs, A, C, fh, fw):
    """head [bs, A (5 + C), fh, fw] of N(0, 4) logits (standard deviation 2) with PLANTED_LOGITS written over every channel kind.  Returns
    (head, planted): `planted` is a bool mask of the same shape."""
    rng = np.random.default_rng(seed)
    x = (2.0 * rng.standard_normal((bs, A, 5 + C, fh * fw))).astype(np.float32)
    planted = np.zeros(x.shape, bool)
    n = fh * fw
    for b in range(bs):
        for a in range(A):
            for k in range(5 + C):
                cells = rng.choice(n, min(n, len(PLANTED_LOGITS)), replace=False)
                vals = rng.permutation(PLANTED_LOGITS)[:len(cells)]
                x[b, a, k, cells] = vals
                planted[b, a, k, cells] = True
    return x.reshape(bs, A * (5 + C), fh, fw), planted.reshape(bs, A * (5 + C), fh, fw)


def decode_f64(head, anchors, C, H, W):
    """val_oracle.decode_head's formulae in float64 on the float32-rounded strides and feature-map anchors that yf_val_decode_head computes
    (yolo_loss.py:52-56 stores Python doubles into FloatTensors).  head: numpy [bs, A (5 + C), fh, fw] -> float64 [bs, A fh fw, 5 + C]."""
    bs, _, fh, fw = head.shape
    A = len(anchors)
    sh, sw = H / fh, W / fw
    aw = np.array([F32(a[0] / sw) for a in anchors], np.float64).reshape(1, A, 1, 1)
    ah = np.array([F32(a[1] / sh) for a in anchors], np.float64).reshape(1, A, 1, 1)
    sw32, sh32 = np.float64(F32(sw)), np.float64(F32(sh))
    p = head.astype(np.float64).reshape(bs, A, 5 + C, fh, fw).transpose(0, 1, 3, 4, 2)
    with np.errstate(over="ignore"):
        sig = 1.0 / (1.0 + np.exp(-p))
        out = np.empty(p.shape, np.float64)
        out[..., 0] = (sig[..., 0] + np.arange(fw, dtype=np.float64).reshape(1, 1, 1, fw)) * sw32
        out[..., 1] = (sig[..., 1] + np.arange(fh, dtype=np.float64).reshape(1, 1, fh, 1)) * sh32
        out[..., 2] = np.exp(p[..., 2]) * aw * sw32
        out[..., 3] = np.exp(p[..., 3]) * ah * sh32
        out[..., 4:] = sig[..., 4:]
    return out.reshape(bs, A * fh * fw, 5 + C)


def ulp_error(got, want64):
    """|got - want64| in units of the fp32 ulp at |want64| (the subnormal spacing 2^-149 below 2^-126); entries whose float32 value is
    infinite are left out (they are compared exactly).  -> float64 array, NaN where left out."""
    want64 = np.asarray(want64, np.float64)
    with np.errstate(over="ignore"):
        w32 = want64.astype(np.float32)
    _, e = np.frexp(np.abs(want64))
    e = np.where(want64 == 0, -1000, e)
    ulp = np.ldexp(1.0, np.maximum(e - 1, -126) - 23)
    err = np.abs(np.asarray(got, np.float64) - want64) / ulp
    err[np.isinf(w32)] = np.nan
    return err
