"""yolov5's autoanchor (utils/autoanchor.py: check_anchors, kmean_anchors, check_anchor_order) for DetectDataset, with the passes over the
label shapes on the device: yf_anchor_metric, yf_anchor_kmeans and yf_anchor_evolve (include/yolo_fastest_hip.h states the rule they
compute).  Opt-in: nothing imports this module unless `training.train(..., autoanchor=True)` or the caller does.

What is yolov5's: the flow, the thresholds (bpr > 0.98 keeps the configured anchors, the new ones are taken only at a greater bpr), the
filter (either side >= 2 px), the metric min(r, 1 / r) in float32, the evolution's draws in their order (numpy's global generator and
`random`: seed both to reproduce a run), its strict acceptance, the sort by area and check_anchor_order.  What is this library's: the
fitness that decides is an exact integer sum, so a decision yolov5's float32 mean would round the other way can differ (tests hold the two
chains equal on a 300-label fixture over 1000 generations); and the k-means that seeds the evolution is the header's lock-step k-means on
quantised labels, `restarts` runs from rows drawn by np.random.choice, the winner picked by fitness -- not scipy's.

This data set squashes every frame to the net input, so yolov5's `shapes` term (the long side scaled to img_size) reduces to the net
input's (W, H): a label's shape is its normalised (w, h) times (W, H)."""
import copy
import ctypes
import logging
import random

import numpy as np
import torch

from . import _lib

PREFIX = "AutoAnchor: "


def _device(device):
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise ValueError("the anchor kernels run on a GPU: device must be a cuda device, got %r" % (device,))
    return torch.device("cuda", torch.cuda.current_device() if device.index is None else device.index)


def _check_host(wh, anchors=None):
    wh = np.ascontiguousarray(wh, np.float32).reshape(-1, 2)
    a = None if anchors is None else np.ascontiguousarray(anchors, np.float32).reshape(-1, 2)
    _lib.check(_lib.lib().yf_anchor_check_host(wh.ctypes.data, len(wh), None if a is None else a.ctypes.data, 0 if a is None else len(a)))
    return wh, a


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _threshold_m(thr):
    t, m = np.float32(1.0 / float(thr)), 0
    while np.float32(2.0 ** -m) > t:
        m += 1
    return m


def label_wh(dataset):
    """float64 [n, 2]: every label's (w, h) in net-input pixels -- DetectDataset._labels' normalised (w, h) times the input (W, H)."""
    H, W = dataset.input_shape[0], dataset.input_shape[1]
    rows = [np.asarray(dataset._labels(i), np.float64).reshape(-1, 5)[:, 3:5] for i in range(len(dataset))]
    wh = np.concatenate(rows) if rows else np.zeros((0, 2))
    return wh * np.array([W, H], np.float64)


def device_sums(wh, anchor_sets, thr=4.0, device=None):
    """int64-valued [S, 3] = (fit, cnt_best, cnt_x) of S anchor sets [S, A, 2] over the labels, in one launch."""
    device = _device(device)
    sets = np.ascontiguousarray(anchor_sets, np.float32)
    S, A = sets.shape[0], sets.shape[1]
    wh, _ = _check_host(wh, sets)
    d_wh, d_k = torch.from_numpy(wh).to(device), torch.from_numpy(sets).to(device)
    out = torch.empty((S, 3), dtype=torch.int64, device=device)
    _lib.check(_lib.lib().yf_anchor_metric(device.index, d_wh.data_ptr(), len(wh), d_k.data_ptr(), S, A, float(thr), out.data_ptr(), _stream(device)))
    return out.cpu().numpy().view(np.uint64)


def anchor_metric(wh, anchors, thr=4.0, device=None):
    """(bpr, aat, fitness) of `anchors` [A, 2] over the label shapes `wh` [n, 2]: yolov5's best possible recall, anchors above the
    threshold per label, and anchor_fitness, as quotients of the device's exact sums."""
    wh = np.asarray(wh, np.float32).reshape(-1, 2)
    fit, cb, cx = (int(x) for x in device_sums(wh, np.asarray(anchors, np.float32).reshape(1, -1, 2), thr, device)[0])
    n = len(wh)
    return cb / n, cx / n, fit / (n * 2.0 ** (23 + _threshold_m(thr)))


def draw_mutations(gen, shape, mp=0.9, sigma=0.1):
    """float64 [gen, *shape]: the mutation factors of kmean_anchors' loop, drawn as yolov5 draws them -- npr.random(shape), random.random(),
    npr.randn(*shape) per attempt, redrawn `while (v == 1).all()`.  They do not depend on the fitness, so the table can be drawn up front."""
    npr = np.random
    shape = tuple(shape)
    out = np.ones((gen,) + shape)
    for g in range(gen):
        v = np.ones(shape)
        while (v == 1).all():
            v = ((npr.random(shape) < mp) * random.random() * npr.randn(*shape) * sigma + 1).clip(0.3, 3.0)
        out[g] = v
    return out


def evolve_passes(accepted, batch=_lib.YF_ANCHOR_BATCH):
    """Passes over the labels yf_anchor_evolve made for this acceptance record (its first pass, for k0's own fitness, included)."""
    gen, g, passes = len(accepted), 0, 1
    while g < gen:
        hits = np.flatnonzero(accepted[g:g + batch])
        g = g + int(hits[0]) + 1 if len(hits) else g + batch
        passes += 1
    return passes


def device_evolve(wh, k0, v, thr=4.0, device=None):
    """yf_anchor_evolve: -> (k float64 [A, 2], fit int, accepted int32 [gen])."""
    device = _device(device)
    k0 = np.ascontiguousarray(k0, np.float64).reshape(-1, 2)
    A = len(k0)
    v = np.ascontiguousarray(v, np.float64).reshape(-1, A, 2)
    wh, _ = _check_host(wh)
    L = _lib.lib()
    d_wh = torch.from_numpy(wh).to(device)
    work = torch.empty(max(int(L.yf_anchor_evolve_work_bytes(A)), 8), dtype=torch.uint8, device=device)
    k_out, fit, acc = np.zeros((A, 2), np.float64), ctypes.c_uint64(0), np.zeros(len(v), np.int32)
    _lib.check(L.yf_anchor_evolve(device.index, d_wh.data_ptr(), len(wh), k0.ctypes.data, v.ctypes.data, A, len(v), float(thr), work.data_ptr(),
                                  work.numel(), k_out.ctypes.data, ctypes.addressof(fit), acc.ctypes.data, _stream(device)))
    return k_out, int(fit.value), acc


def device_kmeans(wh, n, init, thr=4.0, max_iter=100, device=None):
    """yf_anchor_kmeans on float32 label shapes: -> (k float64 [n, 2] or None, winner, iters int32 [R])."""
    device = _device(device)
    wh, _ = _check_host(wh)
    init = np.ascontiguousarray(init, np.int32).reshape(-1, n)
    s = np.ascontiguousarray(wh.std(0), np.float64)
    q = np.rint(wh * np.float32(64.0)).astype(np.int32)
    L = _lib.lib()
    d_wh, d_q = torch.from_numpy(wh).to(device), torch.from_numpy(q).to(device)
    work = torch.empty(max(int(L.yf_anchor_kmeans_work_bytes(len(init), n)), 8), dtype=torch.uint8, device=device)
    k_out, winner, iters = np.zeros((n, 2), np.float64), ctypes.c_int32(-1), np.zeros(len(init), np.int32)
    _lib.check(L.yf_anchor_kmeans(device.index, d_q.data_ptr(), len(wh), s.ctypes.data, init.ctypes.data, len(init), n, int(max_iter), float(thr),
                                  d_wh.data_ptr(), work.data_ptr(), work.numel(), k_out.ctypes.data, ctypes.addressof(winner), iters.ctypes.data,
                                  _stream(device)))
    return (k_out if winner.value >= 0 else None), int(winner.value), iters


def kmean_anchors(dataset_or_wh, n=6, img_size=320, thr=4.0, gen=1000, restarts=30, device=None, logger=None):
    """yolov5's kmean_anchors: `n` anchors fitted to the label shapes of a DetectDataset (or to a [N, 2] array of shapes in pixels).
    -> float32 [n, 2], sorted by area.  Draws, in order: `restarts` x np.random.choice(len(wh), n, replace=False) (or, when n > len(wh) or no
    restart survives, yolov5's random init np.sort(np.random.rand(2 n)).reshape(n, 2) * img_size), then draw_mutations(gen, (n, 2))."""
    logger = logger or logging.getLogger(__name__)
    npr = np.random
    wh0 = label_wh(dataset_or_wh) if hasattr(dataset_or_wh, "_labels") else np.asarray(dataset_or_wh, np.float64).reshape(-1, 2)
    i = int((wh0 < 3.0).any(1).sum())
    if i:
        logger.info("%sWARNING Extremely small objects found: %d of %d labels are <3 pixels in size" % (PREFIX, i, len(wh0)))
    wh = wh0[(wh0 >= 2.0).any(1)].astype(np.float32)
    if len(wh) == 0:
        raise ValueError("no label with a side of at least 2 pixels: nothing to fit anchors to")
    k = None
    logger.info("%sRunning kmeans for %d anchors on %d points..." % (PREFIX, n, len(wh)))
    if n <= len(wh) and (wh.std(0) > 0).all():
        restarts = max(1, min(int(restarts), 1024 // n))
        init = np.stack([npr.choice(len(wh), n, replace=False) for _ in range(restarts)])
        k = device_kmeans(wh, n, init, thr, device=device)[0]
    if k is None:
        logger.warning("%sWARNING switching strategies from kmeans to random init" % PREFIX)
        k = np.maximum(np.sort(npr.rand(n * 2)).reshape(n, 2) * img_size, np.finfo(np.float32).tiny)
    k = k[np.argsort(k.prod(1))]
    if gen > 0:
        k = device_evolve(wh, k, draw_mutations(gen, k.shape), thr, device)[0]
    k = k[np.argsort(k.prod(1))]
    bpr, aat, _ = anchor_metric(wh, k, thr, device)
    logger.info("%sthr=%.2f: %.4f best possible recall, %.2f anchors past thr" % (PREFIX, 1 / thr, bpr, aat))
    logger.info("%sn=%d, img_size=%s: %s" % (PREFIX, n, img_size, ", ".join("%d,%d" % (round(x[0]), round(x[1])) for x in k)))
    return k.astype(np.float32)


def check_anchor_order(anchors, strides):
    """yolov5's check_anchor_order: anchors [nl, na, 2] in pixels; the layers are flipped when the mean anchor area and the strides run in
    opposite directions.  kmean_anchors' result is sorted by area, so this puts ascending areas onto ascending strides."""
    anchors = np.asarray(anchors, np.float32)
    a = anchors.prod(-1).mean(-1)
    da, ds = a[-1] - a[0], strides[-1] - strides[0]
    if da and np.sign(da) != np.sign(ds):
        anchors = anchors[::-1]
    return np.ascontiguousarray(anchors)


def check_anchors(dataset, io_params, thr=4.0, logger=None, device=None):
    """yolov5's check_anchors for this package's io_params: the anchors of the heads in use (io_params["anchors"][:len(strides)]) are
    scored against the data set's label shapes under yolov5's per-image 0.9 - 1.1 jitter (np.random.uniform, one draw per image); at a
    best possible recall above 0.98 they stay, else kmean_anchors fits new ones, taken only if their bpr is greater.  -> a COPY of io_params
    whose "anchors" are the len(strides) groups in use, regrouped by check_anchor_order when they were refitted; the caller's dict is untouched."""
    logger = logger or logging.getLogger(__name__)
    io = copy.deepcopy(io_params)
    nl = len(io["strides"])
    cur = np.asarray(io["anchors"][:nl], np.float32)
    na = cur.shape[1]
    H, W = dataset.input_shape[0], dataset.input_shape[1]
    scale = np.random.uniform(0.9, 1.1, size=(len(dataset), 1))
    rows = [np.asarray(dataset._labels(i), np.float64).reshape(-1, 5)[:, 3:5] * (np.array([W, H], np.float64) * scale[i]) for i in range(len(dataset))]
    wh = (np.concatenate(rows) if rows else np.zeros((0, 2))).astype(np.float32)
    if len(wh) == 0:
        raise ValueError("the data set has no labels: nothing to check the anchors against")
    bpr, aat, _ = anchor_metric(wh, cur.reshape(-1, 2), thr, device)
    s = "\n%s%.2f anchors/target, %.3f Best Possible Recall (BPR). " % (PREFIX, aat, bpr)
    if np.float32(bpr) > np.float32(0.98):                    # yolov5 compares its float32 mean with the scalar in float32
        logger.info("%sCurrent anchors are a good fit to dataset" % s)
        io["anchors"] = cur.tolist()
        return io
    logger.info("%sAnchors are a poor fit to dataset, attempting to improve..." % s)
    new = kmean_anchors(dataset, n=nl * na, img_size=max(H, W), thr=thr, gen=1000, device=device, logger=logger)
    new_bpr = anchor_metric(wh, new, thr, device)[0]
    if np.float32(new_bpr) > np.float32(bpr):
        cur = check_anchor_order(new.reshape(nl, na, 2), io["strides"])
        logger.info("%sDone (optional: update io_params['anchors'] to use these anchors in the future)" % PREFIX)
    else:
        logger.info("%sDone (original anchors better than new anchors, proceeding with original anchors)" % PREFIX)
    io["anchors"] = cur.tolist()
    return io
