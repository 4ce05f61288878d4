"""yolov5's utils/autoanchor.py (v7.0) transcribed in torch on the CPU: check_anchors' metric, kmean_anchors' metric / anchor_fitness and its
evolution loop, check_anchor_order.  scipy is not needed: the k-means result that seeds the evolution is an argument.  A test helper."""
import random

import numpy as np
import torch


def check_metric(wh, k, thr=4.0):
    """check_anchors' inner `metric`: -> (bpr, aat) as float32 tensors, plus best for the tests."""
    wh = torch.as_tensor(np.asarray(wh)).float()
    k = torch.as_tensor(np.asarray(k)).float()
    r = wh[:, None] / k[None]
    x = torch.min(r, 1 / r).min(2)[0]  # ratio metric
    best = x.max(1)[0]  # best_x
    aat = (x > 1 / thr).float().sum(1).mean()  # anchors above threshold
    bpr = (best > 1 / thr).float().mean()  # best possible recall
    return bpr, aat, best


def draw_mutations(gen, sh, mp=0.9, s=0.1):
    """The v tables of kmean_anchors' loop, drawn as it draws them (numpy's global generator and `random`)."""
    npr = np.random
    out = []
    for _ in range(gen):
        v = np.ones(sh)
        while (v == 1).all():  # mutate until a change occurs (prevent duplicates)
            v = ((npr.random(sh) < mp) * random.random() * npr.randn(*sh) * s + 1).clip(0.3, 3.0)
        out.append(v)
    return np.stack(out) if out else np.ones((0,) + tuple(sh))


def evolve(wh, k, thr=4.0, gen=1000, v=None):
    """kmean_anchors from `# Evolve` on: wh float32 [n,2] (already filtered), k float64 [A,2] (already sorted by area).  With v=None the
    mutations are drawn inside the loop, as yolov5 does; with a table they are read from it.  -> (k, accepted generations, f)."""
    npr = np.random
    thr = 1 / thr
    wh = torch.tensor(np.asarray(wh), dtype=torch.float32)

    def metric(k, wh):  # compute metrics
        r = wh[:, None] / k[None]
        x = torch.min(r, 1 / r).min(2)[0]  # ratio metric
        return x, x.max(1)[0]  # x, best_x

    def anchor_fitness(k):  # mutation fitness
        _, best = metric(torch.tensor(k, dtype=torch.float32), wh)
        return (best * (best > thr).float()).mean()  # fitness

    k = np.array(k, np.float64)
    f, sh, mp, s = anchor_fitness(k), k.shape, 0.9, 0.1  # fitness, generations, mutation prob, sigma
    acc = []
    for g in range(gen):
        if v is None:
            vg = np.ones(sh)
            while (vg == 1).all():  # mutate until a change occurs (prevent duplicates)
                vg = ((npr.random(sh) < mp) * random.random() * npr.randn(*sh) * s + 1).clip(0.3, 3.0)
        else:
            vg = v[g]
        kg = (k.copy() * vg).clip(min=2.0)
        fg = anchor_fitness(kg)
        if fg > f:
            f, k = fg, kg.copy()
            acc.append(g)
    return k[np.argsort(k.prod(1))], acc, f


def check_anchor_order(anchors, strides):
    """check_anchor_order on anchors float [nl, na, 2] (pixels) and strides [nl]: -> the anchors, flipped along the layers if the mean
    anchor area and the strides run in opposite directions."""
    anchors = torch.as_tensor(np.asarray(anchors, np.float32))
    stride = torch.as_tensor(np.asarray(strides, np.float32))
    a = anchors.prod(-1).mean(-1).view(-1)  # mean anchor area per output layer
    da = a[-1] - a[0]  # delta a
    ds = stride[-1] - stride[0]  # delta s
    if da and (da.sign() != ds.sign()):  # same order
        anchors = anchors.flip(0)
    return anchors.numpy()
