"""Decode + NMS (post_kernel / post_split_kernel + post_assemble_kernel) at other (num_cls, num_anchors) than the shipped (3, 3), bit for
bit against oracle/post_oracle.c (the reference's loop, restated) on random logit fields.

tests/test_gpu_parity.py test_post_process_randomised_against_c_oracle runs this battery -- sparse to very dense fields, nms_thres 0, 1 and
negative, a low conf_thres, quantised logits (exact ties in confidence and between classes), zero-area boxes (the reference's
ZeroDivisionError: count -2) -- with 3 classes and 3 anchors only; other io_params saw the reference's two golden frames.  Here the same
fields with (A, 5 + C) channels (io_cfg.post_fields; tests/test_cpu_io_post.py holds the generator to the oracle alone), 256x320, three
frames per case, kmax = the cell count:

  (C, A)             post_split   why
  (1, 3)             2 and 1      one class: every candidate in one bucket
  (8, 3), (9, 3)     0            the automatic rule's boundary: the per-class form at 8 classes, the per-frame form at 9
  (20, 3)            2 and 1      a forced split beyond 8 classes
  (64, 1), (65, 2)   1            the split's own limit, and the fall-back to the per-frame form above it (post_setup: `nc > 64`)
  (2, 8), (3, 2)     2 and 1      most anchors (3200 cells), fewer than shipped
  (80, 3)            2            the widest shipped-style head

Which form ran is asserted from the engine (`yf_post_dispatches`: 2 = post_split_kernel + the assembly launch, 1 = post_kernel)."""
import ctypes
from collections import OrderedDict

import numpy as np
import pytest
import torch

from tests import io_cfg

pytestmark = pytest.mark.gpu

PARAMS = [(C, A, mode) for C, A, modes in io_cfg.POST_CONFIGS for mode in modes]
_MODELS = {}


@pytest.fixture(scope="module")
def yf():
    import yolo_fastest_amd
    return yolo_fastest_amd


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _model(yf, dev, C, A):
    if (C, A) not in _MODELS:
        io = io_cfg.post_io(C, A)
        m = yf.YoloFastest(io)
        sd = OrderedDict((k, torch.from_numpy(np.asarray(v))) for k, v in io_cfg.seeded_state_dict(
            OrderedDict((k, tuple(v.shape)) for k, v in m.state_dict().items()), 77).items())
        m.load_state_dict(sd)
        _MODELS[(C, A)] = (m.to(dev).eval(), io)
    return _MODELS[(C, A)]


def _split_expected(mode, C, kmax, N, n_cu):
    """yf_engine.hip post_setup, restated: 1 = always (up to 64 classes), 2 = never, 0 = kmax >= 256, at most 8 classes and 2 N <= #CU."""
    on = mode == 1 or (mode == 0 and kmax >= 256 and C <= 8 and 2 * N <= n_cu)
    return on and C <= 64


@pytest.mark.parametrize("C,A,mode", PARAMS, ids=lambda v: str(v))
def test_post_process_randomised_against_c_oracle_for_other_io_params(yf, dev, C, A, mode):
    from oracle import post_oracle_c as poc
    m, io = _model(yf, dev, C, A)
    assert m.num_out == A * (5 + C)
    H, W, N = io_cfg.POST_H, io_cfg.POST_W, io_cfg.POST_FRAMES
    kmax = A * (H // 16 * (W // 16) + H // 32 * (W // 32))
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    m.post_split = mode
    try:
        e = m.engine(H, W, N, dev)
        nd = ctypes.c_int()
        yf._lib.check(e.lib.yf_post_dispatches(e.handle, N, kmax, ctypes.byref(nd)))
        want_split = _split_expected(mode, C, kmax, N, n_cu)
        assert nd.value == (2 if want_split else 1), (C, A, mode, nd.value)
        assert want_split == {(8, 0): True, (9, 0): False, (64, 1): True, (65, 1): False}.get((C, mode), mode == 1)
        raised = compared = 0
        for ci, (conf, nms, mu, sd, wh_mu, quant) in enumerate(io_cfg.POST_THRESHOLDS):
            hl, hs = io_cfg.post_fields(C, A, ci)
            post = yf.YOLO_post_process(conf, nms, A, C, io["anchors"], io["input_shape"]).bind(m)
            pred = (torch.from_numpy(np.stack(hl)).to(dev), torch.from_numpy(np.stack(hs)).to(dev))
            raw = post.detect_raw(pred, kmax=kmax)
            counts = raw["counts"].cpu().numpy()
            for f in range(N):
                try:
                    r = poc.post_process(hl[f], hs[f], io["anchors"], io["input_shape"][:2], conf_thres=conf, nms_thres=nms, num_cls=C, num_anchors=A)
                except ZeroDivisionError:       # the reference raises (detect.py:39): the kernel reports count -2
                    assert counts[f] == -2, (C, A, mode, ci, f, counts[f])
                    raised += 1
                    continue
                n = r["count"]
                assert counts[f] == n, (C, A, mode, ci, f, counts[f], n, r["n_candidates"])
                compared += n
                assert np.array_equal(raw["src"][f, :n].cpu().numpy(), r["src"]), (C, A, mode, ci, f)
                assert np.array_equal(raw["boxes"][f, :n].cpu().numpy(), r["box"]), (C, A, mode, ci, f)
                assert np.array_equal(raw["cls"][f, :n].cpu().numpy(), r["cls"]), (C, A, mode, ci, f)
                sc = raw["scores"][f, :n].cpu().numpy().astype(np.float64)
                assert n == 0 or (np.abs(sc[:, 0] - r["conf"]).max() < 1e-6 and np.abs(sc[:, 1] - r["score"]).max() < 1e-6)
        assert raised == 1 and compared > 1000, (raised, compared)     # the tiny-box case's one frame; tests/test_cpu_io_post.py
    finally:
        m.post_split = 0
