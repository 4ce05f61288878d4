"""Fixtures shared by tests/test_cpu_anchors.py and tests/test_gpu_anchors.py: label shapes, anchor sets and the evolution's seed."""
import functools
import random

import numpy as np

import anchor_ref
import anchor_v5_ref

BASES = np.array([[20, 12], [60, 40], [150, 110]], float)


def lognormal_labels(n_lab, seed=0):
    """Three log-normal shape clusters, then yolov5's filter (either side >= 2 px): float32 [<= n_lab, 2]."""
    rs = np.random.RandomState(seed)
    c = rs.randint(0, 3, n_lab)
    wh0 = BASES[c] * np.exp(rs.randn(n_lab, 2) * 0.35)
    return wh0[(wh0 >= 2.0).any(1)].astype(np.float32)


# labels the metric must get right whatever surrounds them
EDGE_LABELS = np.array([
    [1.0, 1000.0],    # against anchor (3, 1000), out of the other anchors' reach: x = (float)(1 / 3) exactly -- not above t at thr 3 in
                      # float32, above 1 / 3 as a double
    [2.0, 8.0],       # against anchor (8, 8): x = 0.25 exactly -- not above t at thr 4
    [0.0, 40.0],      # a zero side: x = 0 against every anchor
    [8.0, 8.0],       # x = 1 against (8, 8): the largest term, 2^(23+m)
    [3.0, 5.0],
], np.float32)
EDGE_ANCHORS = np.array([[3.0, 1000.0], [8.0, 8.0]], np.float32)


def metric_labels(n, seed=3):
    """float32 [n, 2]: the edge labels first (as many as fit), log-normal shapes behind them."""
    wh = np.concatenate([EDGE_LABELS, lognormal_labels(n + 16, seed)])[:n]
    assert len(wh) == n
    return np.ascontiguousarray(wh)


def anchor_sets(S, A, seed=5):
    """float32 [S, A, 2]: set 0 starts with the edge anchors (as many as fit), the rest log-uniform in [2, 300)."""
    rs = np.random.RandomState(seed)
    k = np.exp(rs.uniform(np.log(2.0), np.log(300.0), size=(S, A, 2))).astype(np.float32)
    m = min(A, len(EDGE_ANCHORS))
    k[0, :m] = EDGE_ANCHORS[:m]
    return k


@functools.lru_cache(maxsize=None)
def evolution_fixture():
    """The 300-label fixture of the evolution tests: (wh float32 [n,2], k0 float64 [6,2] sorted by area, v float64 [1000,6,2]).  k0 is the
    rule's own k-means from six drawn rows; v is yolov5's draw sequence under np.random.seed(0), random.seed(0)."""
    wh = lognormal_labels(300, 0)
    s = wh.std(0).astype(np.float64)
    init = np.random.RandomState(1).choice(len(wh), 6, replace=False)[None]
    k, winner, _ = anchor_ref.kmeans(anchor_ref.quantise(wh), s, init, 100, wh, 4.0)
    assert winner == 0
    k = k[np.argsort(k.prod(1))]
    state = (np.random.get_state(), random.getstate())
    np.random.seed(0)
    random.seed(0)
    v = anchor_v5_ref.draw_mutations(1000, k.shape)
    np.random.set_state(state[0])
    random.setstate(state[1])
    return wh, k, v


@functools.lru_cache(maxsize=None)
def evolution_reference():
    """anchor_ref's chain on the fixture, computed once: (k, fit, accepted)."""
    wh, k, v = evolution_fixture()
    return anchor_ref.evolve(wh, k, v, 4.0)
