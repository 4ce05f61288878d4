"""Shared by the CPU oracle tests and the GPU tests of the io_params generality: the configurations of
tests/golden/seeded_weights.IO_CONFIGS, their io_params dicts and their numpy-seeded state-dicts (golden_io.npz holds what the
REFERENCE computed for exactly these weights and inputs)."""
import copy
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from seeded_weights import IO_CONFIGS, io_inputs, io_targets, seeded_state_dict  # noqa: E402,F401

CONFIG = {tag: (C, Cin, A) for tag, C, Cin, A in IO_CONFIGS}
TAGS = [c[0] for c in IO_CONFIGS]


def io_for(tag, H=256, W=320):
    import yolo_fastest_amd as yf
    C, Cin, A = CONFIG[tag]
    io = copy.deepcopy(yf.config_params["io_params"])
    io.update(num_cls=C, input_channel=Cin, num_anchors=A, input_shape=[H, W, Cin], origin_img_shape=[H, W, Cin],
              anchors=[grp[:A] for grp in yf.config_params["io_params"]["anchors"]], class_names=["c%d" % i for i in range(C)])
    return io


def state_dict_for(tag, seed):
    """The state-dict make_golden.py loaded into the reference module: keys, order and shapes from THIS package's module (a strict
    load into the reference's module succeeded with the same key set), values from the numpy stream of `seed`."""
    import yolo_fastest_amd as yf
    m = yf.YoloFastest(io_for(tag))
    shapes = OrderedDict((k, tuple(v.shape)) for k, v in m.state_dict().items())
    return OrderedDict((k, torch.from_numpy(np.asarray(v))) for k, v in seeded_state_dict(shapes, seed).items())


# ---- decode + NMS at other (num_cls, num_anchors): tests/test_cpu_io_post.py (the generator, C oracle only), tests/test_gpu_io_post.py ----
#
# tests/test_gpu_parity.py test_post_process_randomised_against_c_oracle's random logit fields and its eight threshold / quantisation
# cases, generalised to (A, 5 + C) channels.  (C, A) -> the post_split modes to run (0 auto, 1 per frame and class, 2 per frame):
POST_CONFIGS = [
    (1, 3, (2, 1)),        # one class: every candidate in one bucket
    (8, 3, (0,)),          # the automatic rule's boundary: the per-class form at 8 classes ...
    (9, 3, (0,)),          # ... the per-frame form at 9
    (20, 3, (2, 1)),       # a forced split beyond 8 classes
    (64, 1, (1,)),         # the split's own limit
    (65, 2, (1,)),         # ... and the fall-back to the per-frame form above it
    (2, 8, (2, 1)),        # most anchors: 3200 cells
    (3, 2, (2, 1)),        # fewer anchors than shipped
    (80, 3, (2,)),         # the widest shipped-style head
]
POST_H, POST_W, POST_FRAMES = 256, 320, 3
# (conf_thres, nms_thres, mu and sd of the objectness logit, mu of the t_w / t_h logits, quantum of objectness and class logits or None):
# sparse to very dense, nms_thres 0 / 1 / negative (where even disjoint boxes suppress each other), a low conf_thres, quantised logits (exact
# ties in confidence and between classes), tiny boxes (zero area: the reference's ZeroDivisionError, count -2)
POST_THRESHOLDS = [(0.5, 0.2, -1.0, 1.5, 0.5, None), (0.5, 0.0, -1.0, 1.5, 0.5, None), (0.5, 1.0, -2.0, 1.0, 0.5, None),
                   (0.5, -0.1, -2.5, 1.0, 0.5, None), (0.2, 0.5, 0.0, 2.0, 1.0, None), (0.5, 0.3, -1.0, 1.5, 0.5, 0.5),
                   (0.5, 0.2, -2.0, 1.0, -6.0, None), (0.9, 0.45, 1.0, 2.0, 0.3, 1.0)]
TINY = 6     # the tiny-box case: its wh_mu is chosen per (C, A) so that the oracle raises for at most one frame in three (a case that raises
             # for all three tests nothing): more cells per class bucket need larger boxes.  tests/test_cpu_io_post.py asserts the choice.
POST_TINY_WH_MU = {(1, 3): -2.0, (8, 3): -2.75, (9, 3): -2.5, (20, 3): -2.5, (64, 1): -3.0, (65, 2): -4.0, (2, 8): -2.25, (3, 2): -2.75, (80, 3): -3.25}


def post_anchors(A):
    """Shipped anchors cut to A per scale; eight per scale as in test_gpu_io_params.test_eight_anchors_and_the_cell_limit."""
    import yolo_fastest_amd as yf
    if A <= 3:
        return [grp[:A] for grp in yf.config_params["io_params"]["anchors"]]
    return [[[10 + 7 * k, 13 + 5 * k] for k in range(A)], [[40 + 20 * k, 150 - 15 * k] for k in range(A)], [[1, 1]] * A]


def post_io(C, A):
    import yolo_fastest_amd as yf
    io = copy.deepcopy(yf.config_params["io_params"])
    io.update(num_cls=C, num_anchors=A, anchors=post_anchors(A), class_names=["c%d" % i for i in range(C)])
    return io


def post_fields(C, A, ci, wh_mu=None):
    """The POST_FRAMES logit fields of threshold case ci: ([head_large [A (5 + C), 16, 20]], [head_small [.., 8, 10]]).  Quantised cases: the
    class logits are quantised AND capped two quanta above zero, so that with many classes several share the maximum (first one wins)."""
    conf, nms, mu, sd, whm, quant = POST_THRESHOLDS[ci]
    if wh_mu is None:
        wh_mu = POST_TINY_WH_MU.get((C, A), whm) if ci == TINY else whm
    hl, hs = [], []
    for f in range(POST_FRAMES):
        g = np.random.default_rng(1000 * ci + f + 100003 * C + 7 * A)
        for (h, w), dst in (((POST_H // 16, POST_W // 16), hl), ((POST_H // 32, POST_W // 32), hs)):
            t = np.empty((A, 5 + C, h, w), np.float32)
            t[:, 0:2] = g.normal(0.0, 1.0, (A, 2, h, w)); t[:, 2:4] = g.normal(wh_mu, 0.5, (A, 2, h, w))
            t[:, 4] = g.normal(mu, sd, (A, h, w)); t[:, 5:] = g.normal(0.0, 2.0, (A, C, h, w))
            if quant:
                t[:, 4:] = np.round(t[:, 4:] / quant) * quant
                t[:, 5:] = np.minimum(t[:, 5:], 2 * quant)
            dst.append(t.reshape(A * (5 + C), h, w))
    return hl, hs


def post_class_ties(head, C, A, conf_thres):
    """Candidate cells of one head whose largest class logit is shared by two or more classes."""
    t = head.reshape(A, 5 + C, -1)
    cand = 1.0 / (1.0 + np.exp(-t[:, 4].astype(np.float64))) > conf_thres
    top = t[:, 5:].max(1, keepdims=True)
    return int((((t[:, 5:] == top).sum(1) > 1) & cand).sum())


def unpack_lists(g, prefix, f):
    """frame f of pack_lists' arrays -> dict of trimmed arrays (count -2: the reference raised ZeroDivisionError)."""
    n = int(g[prefix + "_count"][f])
    m = max(n, 0)
    return dict(count=n, box=g[prefix + "_box"][f, :m], conf=g[prefix + "_conf"][f, :m], score=g[prefix + "_score"][f, :m],
                cls=g[prefix + "_cls"][f, :m], src=g[prefix + "_src"][f, :m])
