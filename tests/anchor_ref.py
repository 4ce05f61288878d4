"""The autoanchor rule of include/yolo_fastest_hip.h in numpy: float32 arithmetic, int64 sums, the sequential chain, the lock-step k-means.
A test helper: the device entries (yf_anchor_metric / _evolve / _kmeans) are held to this bit for bit, and this to tests/anchor_v5_ref.py's
transcription of yolov5."""
import numpy as np


def threshold(thr):
    """-> (t, m): t = (float)(1.0 / thr), m the smallest integer with 2^-m <= t."""
    t = np.float32(1.0 / float(thr))
    m = 0
    while np.float32(2.0 ** -m) > t:
        m += 1
    return t, m


def ratio_x(wh, k):
    """x float32 [n, A]: min(min(rw, 1 / rw), min(rh, 1 / rh)), 1 / r a second division of the quotient."""
    wh = np.asarray(wh, np.float32).reshape(-1, 2)
    k = np.asarray(k, np.float32).reshape(-1, 2)
    with np.errstate(divide="ignore", over="ignore", under="ignore"):
        r = wh[:, None, :] / k[None, :, :]
        inv = np.float32(1.0) / r
    return np.minimum(r, inv).min(2)


def sums(wh, k, thr):
    """-> (fit, cnt_best, cnt_x) as Python ints, and best float32 [n]."""
    t, m = threshold(thr)
    x = ratio_x(wh, k)
    best = x.max(1)
    hit = best > t
    terms = best[hit].astype(np.float64) * 2.0 ** (23 + m)
    assert (terms == np.rint(terms)).all() and (terms <= 2.0 ** 31).all()
    return (int(terms.astype(np.int64).sum()), int(hit.sum()), int((x > t).sum())), best


def fit(wh, k, thr):
    return sums(wh, k, thr)[0][0]


def metric(wh, k, thr):
    """(bpr, aat, anchor_fitness) as Python floats (float64 quotients of the integer sums)."""
    (f, cb, cx), _ = sums(wh, k, thr)
    n = len(np.asarray(wh).reshape(-1, 2))
    _, m = threshold(thr)
    return cb / n, cx / n, f / (n * 2.0 ** (23 + m))


def evolve(wh, k0, v, thr):
    """The sequential chain: -> (k float64 [A,2], f int, accepted list of generations)."""
    k = np.array(k0, np.float64)
    f = fit(wh, k.astype(np.float32), thr)
    acc = []
    for g in range(len(v)):
        kg = np.maximum(k * np.asarray(v[g], np.float64), 2.0)
        fg = fit(wh, kg.astype(np.float32), thr)
        if fg > f:
            f, k = fg, kg
            acc.append(g)
    return k, f, acc


def quantise(wh):
    return np.rint(np.asarray(wh, np.float32) * np.float32(64.0)).astype(np.int32)


def kmeans(q, s, init, max_iter, wh, thr):
    """-> (k float64 [A,2] or None, winner, iters int32 [R]).  q int32 [n,2], s two doubles, init int [R,A]."""
    q = np.asarray(q, np.int32)
    s = np.asarray(s, np.float64)
    init = np.asarray(init).reshape(len(init), -1)
    R, A = init.shape
    obs = (q.astype(np.float64) / 64.0) / s
    iters = np.zeros(R, np.int32)
    cents = [None] * R
    for r in range(R):
        c = obs[init[r]].copy()
        prev = None
        for it in range(1, max_iter + 1):
            dw = obs[:, None, 0] - c[None, :, 0]
            dh = obs[:, None, 1] - c[None, :, 1]
            d = dw * dw + dh * dh
            lab = d.argmin(1)                                   # the first index among equals
            tri = np.zeros((A, 3), np.int64)
            np.add.at(tri[:, 0], lab, q[:, 0].astype(np.int64))
            np.add.at(tri[:, 1], lab, q[:, 1].astype(np.int64))
            np.add.at(tri[:, 2], lab, 1)
            if (tri[:, 2] == 0).any():
                iters[r] = -1
                break
            iters[r] = it
            c = (tri[:, :2].astype(np.float64) / (64.0 * tri[:, 2:3].astype(np.float64))) / s
            same = prev is not None and np.array_equal(prev, tri)
            prev = tri
            if same:
                break
        if iters[r] >= 0:
            kf = (c * s).astype(np.float32)
            if np.isfinite(kf).all() and (kf > 0).all():
                cents[r] = c
            else:
                iters[r] = -1
    winner, best = -1, -1
    for r in range(R):
        if cents[r] is not None:
            f = fit(wh, (cents[r] * s).astype(np.float32), thr)
            if f > best:
                winner, best = r, f
    return (cents[winner] * s if winner >= 0 else None), winner, iters
