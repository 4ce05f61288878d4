"""The generator of tests/test_gpu_io_post.py (io_cfg.post_fields: random logit fields at other (num_cls, num_anchors) under eight threshold /
quantisation cases), on the C oracle alone.  What the GPU test compares bit for bit must be worth comparing:
  * a threshold case in which the oracle raises ZeroDivisionError (two zero-area boxes compared, detect.py:39) for all three frames tests
    nothing but the count -2: at most one frame in three raises, in every case of every configuration, and in the tiny-box case exactly one
    does (io_cfg.POST_TINY_WH_MU is chosen so);
  * every configuration has a frame with more than 50 survivors, and quantised cases with ties: survivors of one class with equal
    confidence (the stable sort keeps their order) and, with more than one class, candidate cells whose largest class logit is shared
    (first maximum wins)."""
import numpy as np
import pytest

from oracle import post_oracle_c as poc
from tests import io_cfg


@pytest.mark.parametrize("C,A,modes", io_cfg.POST_CONFIGS, ids=lambda v: str(v))
def test_generator_gives_the_oracle_something_to_decide(C, A, modes):
    anchors = io_cfg.post_anchors(A)
    assert len(anchors[0]) == len(anchors[1]) == A and A * (5 + C) >= 1
    most, conf_ties, class_ties = 0, 0, 0
    for ci, (conf, nms, mu, sd, wh_mu, quant) in enumerate(io_cfg.POST_THRESHOLDS):
        hl, hs = io_cfg.post_fields(C, A, ci)
        assert len(hl) == io_cfg.POST_FRAMES and hl[0].shape == (A * (5 + C), 16, 20) and hs[0].shape == (A * (5 + C), 8, 10)
        raised = 0
        for f in range(io_cfg.POST_FRAMES):
            try:
                r = poc.post_process(hl[f], hs[f], anchors, [io_cfg.POST_H, io_cfg.POST_W], conf, nms, C, num_anchors=A)
            except ZeroDivisionError:
                raised += 1
                continue
            most = max(most, r["count"])
            assert r["count"] <= r["n_candidates"] <= A * 400 and (r["count"] == 0 or 0 <= r["cls"].min() <= r["cls"].max() < C)
            if quant:
                conf_ties += r["count"] - len(set(zip(r["cls"].tolist(), r["conf"].tolist())))
                class_ties += io_cfg.post_class_ties(hl[f], C, A, conf) + io_cfg.post_class_ties(hs[f], C, A, conf)
        assert raised <= 1, (C, A, ci, raised)
        assert ci != io_cfg.TINY or raised == 1, (C, A, raised)
    print("(%d classes, %d anchors): most survivors %d, survivors tied in confidence %d, candidate cells with tied classes %d" % (C, A, most, conf_ties, class_ties))
    assert most > 50 and conf_ties > 0 and (C == 1 or class_ties > 0)


def test_configurations_are_the_documented_ones():
    assert [(c, a) for c, a, _ in io_cfg.POST_CONFIGS] == [(1, 3), (8, 3), (9, 3), (20, 3), (64, 1), (65, 2), (2, 8), (3, 2), (80, 3)]
    assert set(io_cfg.POST_TINY_WH_MU) == {(c, a) for c, a, _ in io_cfg.POST_CONFIGS} and len(io_cfg.POST_THRESHOLDS) == 8
    assert np.asarray(io_cfg.post_anchors(8)).shape == (3, 8, 2) and 8 * 400 == 3200
