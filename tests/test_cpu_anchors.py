"""Autoanchor on the host (anchors.py, include/yolo_fastest_hip.h): the rule's numpy statement (tests/anchor_ref.py) against
the transcription of yolov5 (tests/anchor_v5_ref.py) bit for bit, the draws, the label shapes, the anchor order, and the C entries'
declarations and refusals.  No GPU needed: every refusal comes back before a device is touched."""
import ctypes
import logging
import os
import random
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import anchor_cases  # noqa: E402
import anchor_ref  # noqa: E402
import anchor_v5_ref  # noqa: E402
import voc_tree  # noqa: E402
from yolo_fastest_amd import _lib  # noqa: E402
from yolo_fastest_amd import anchors as aa  # noqa: E402
from yolo_fastest_amd.dataset import DetectDataset  # noqa: E402

LOG = logging.getLogger("test-anchors")
ENTRIES = ("yf_anchor_check_host", "yf_anchor_metric", "yf_anchor_evolve", "yf_anchor_evolve_work_bytes", "yf_anchor_kmeans",
           "yf_anchor_kmeans_work_bytes")


# ---- the rule against yolov5 ----
@pytest.mark.parametrize("thr", [4.0, 3.0])
def test_metric_is_yolov5s_bit_for_bit(thr):
    """bpr, aat and every label's best.  At thr 3 the label (1, 1000) has best = (float)(1 / 3), which is above the double 1 / 3 and not above
    the float: torch compares in float32, and so does the rule."""
    wh = anchor_cases.metric_labels(5003)
    k = anchor_cases.anchor_sets(1, 6)[0]
    (fit, cb, cx), best = anchor_ref.sums(wh, k, thr)
    bpr, aat, vbest = anchor_v5_ref.check_metric(wh, k, thr)
    assert np.array_equal(best.view(np.uint32), vbest.numpy().view(np.uint32))
    n = len(wh)
    assert np.float32(cb / n) == np.float32(bpr.item()) and np.float32(cx / n) == np.float32(aat.item())
    assert cb == int((vbest > 1 / thr).sum()) and 0 < cb < n
    if thr == 3.0:
        assert best[0] == np.float32(1.0 / 3.0) and float(best[0]) > 1.0 / 3.0         # the case that settles the comparison
        assert not bool(vbest[0] > 1 / thr)
    t, m = anchor_ref.threshold(thr)
    assert m == 2 and (thr != 4.0 or t == 0.25)
    # anchor_fitness is the same mean up to float32 summation: the integer sum is the exact value of what yolov5 rounds
    v5_fitness = float((vbest * (vbest > 1 / thr).float()).mean())
    assert abs(anchor_ref.metric(wh, k, thr)[2] - v5_fitness) < 1e-5


def test_threshold_edges():
    assert [anchor_ref.threshold(t)[1] for t in (1, 2, 3, 4, 5, 255, 256)] == [0, 1, 2, 2, 3, 8, 8]
    wh = anchor_cases.EDGE_LABELS
    (fit, cb, cx), best = anchor_ref.sums(wh, anchor_cases.EDGE_ANCHORS, 4.0)
    assert best[1] == 0.25 and best[2] == 0.0 and best[3] == 1.0      # on the threshold; a zero side; an exact fit
    assert anchor_ref.sums(wh, anchor_cases.EDGE_ANCHORS, 1.0)[0] == (0, 0, 0)       # thr 1: nothing is above 1
    assert anchor_ref.sums(wh[3:4], anchor_cases.EDGE_ANCHORS[1:], 256.0)[0] == (2 ** 31, 1, 1)   # the largest term there is


def test_the_division_shortcut_changes_the_fit():
    """1 / r is a division of the rounded quotient.  The fixture holds pairs where aw / w rounds differently, and they move fit: a kernel
    that takes the shortcut cannot pass the device tests on these labels."""
    wh = anchor_cases.metric_labels(5003)
    k = anchor_cases.anchor_sets(1, 6)[0]
    with np.errstate(divide="ignore"):
        r = wh[:, None, :] / k[None, :, :]
        rule = np.float32(1.0) / r
        shortcut = k[None, :, :] / wh[:, None, :]
    assert (rule != shortcut).any()
    t, m = anchor_ref.threshold(4.0)
    best = np.minimum(r, shortcut).min(2).max(1)
    hit = best > t
    short_fit = int((best[hit].astype(np.float64) * 2.0 ** (23 + m)).astype(np.int64).sum())
    assert short_fit != anchor_ref.fit(wh, k, 4.0)


def test_evolution_is_yolov5s_chain_over_1000_generations():
    """The transcription means in float32 and the rule sums exactly; on this fixture no decision lies within that rounding: the accepted
    generations and the final anchors are identical."""
    wh, k0, v = anchor_cases.evolution_fixture()
    k, f, acc = anchor_cases.evolution_reference()
    vk, vacc, vf = anchor_v5_ref.evolve(wh, k0, 4.0, len(v), v=v)
    assert len(v) == 1000 and len(acc) > 20
    assert acc == vacc
    assert np.array_equal(k[np.argsort(k.prod(1))], vk)
    assert abs(f / (len(wh) * 2.0 ** 25) - float(vf)) < 1e-6


# ---- the draws ----
def test_draw_mutations_is_yolov5s_sequence():
    wh, k0, v = anchor_cases.evolution_fixture()
    np.random.seed(0)
    random.seed(0)
    mine = aa.draw_mutations(1000, k0.shape)
    assert np.array_equal(mine, v)
    assert ((mine >= 0.3) & (mine <= 3.0)).all() and not (mine == 1).all(axis=(1, 2)).any()
    # drawn inside the loop, as yolov5 does, the chain is the same: no draw depends on an outcome
    np.random.seed(0)
    random.seed(0)
    vk, vacc, _ = anchor_v5_ref.evolve(wh, k0, 4.0, 200)
    assert vacc == [g for g in anchor_cases.evolution_reference()[2] if g < 200]
    np.random.seed(7)
    random.seed(7)
    a = aa.draw_mutations(5, (9, 2), mp=0.5, sigma=0.3)
    np.random.seed(7)
    random.seed(7)
    assert np.array_equal(a, anchor_v5_ref.draw_mutations(5, (9, 2), mp=0.5, s=0.3))


def test_evolve_passes_counts_the_batches():
    acc = np.zeros(70, np.int32)
    assert aa.evolve_passes(acc, 32) == 1 + 3
    acc[[0, 31, 40]] = 1                              # pass at 0 -> resumes at 1; 1..32 hits 31 -> 32; 32..63 hits 40 -> 41; 41..69
    assert aa.evolve_passes(acc, 32) == 1 + 4


@pytest.fixture()
def train_ds(tmp_path):
    trees = voc_tree.make_trees(tmp_path)
    ds = DetectDataset([256, 320, 1], [512, 640, 3], LOG, aug_params=voc_tree.aug_params(trees), max_boxes=64, device="cpu")
    ds.img_list.sort()
    return ds


def test_label_wh_against_the_xml(train_ds):
    """syn_linear.xml's three boxes by hand: (xmax - xmin) / 640 * 320, (ymax - ymin) / 512 * 256 (the CONFIGURED origin shape normalises)."""
    wh = aa.label_wh(train_ds)
    counts = [len(train_ds._labels(i)) for i in range(len(train_ds))]
    assert wh.dtype == np.float64 and wh.shape == (sum(counts), 2)
    i = [os.path.basename(p) for p in train_ds.img_list].index("syn_linear.jpg")
    lo = sum(counts[:i])
    assert counts[i] == 3 and np.array_equal(wh[lo:lo + 3], [[16.5, 11.5], [15.0, 4.0], [10.0, 18.5]])
    j = [os.path.basename(p) for p in train_ds.img_list].index("syn_empty.jpg")
    assert counts[j] == 0


def test_check_anchor_order_and_regrouping():
    k = np.array([[10, 10], [20, 20], [30, 30], [40, 40], [50, 50], [60, 60]], np.float32)
    for strides in ([16, 32], [32, 16], [16, 16]):
        mine = aa.check_anchor_order(k.reshape(2, 3, 2), strides)
        assert np.array_equal(mine, anchor_v5_ref.check_anchor_order(k.reshape(2, 3, 2), strides))
    assert np.array_equal(aa.check_anchor_order(k.reshape(2, 3, 2), [16, 32])[0], k[:3])      # ascending areas onto ascending strides
    assert np.array_equal(aa.check_anchor_order(k.reshape(2, 3, 2), [32, 16])[0], k[3:])
    assert np.array_equal(aa.check_anchor_order(k[::-1].reshape(2, 3, 2), [16, 32])[1], k[::-1][:3])


# ---- the C ABI ----
def test_abi_declares_binds_and_exports_the_entries():
    hdr = open(os.path.join(ROOT, "include", "yolo_fastest_hip.h")).read()
    L = _lib.lib()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert "#define YF_ANCHOR_BATCH %d" % _lib.YF_ANCHOR_BATCH in hdr and "#define YF_ANCHOR_MAX_A %d" % _lib.YF_ANCHOR_MAX_A in hdr
    assert "#define YF_ABI_VERSION 1" in hdr and L.yf_abi_version() == 1
    G = _lib.YF_ANCHOR_BATCH
    for A in (1, 6, 32):
        assert L.yf_anchor_evolve_work_bytes(A) == G * A * 8 + G * 24            # candidates float32 [G,A,2], sums uint64 [G,3]
    assert L.yf_anchor_evolve_work_bytes(0) == 0 and L.yf_anchor_evolve_work_bytes(33) == 0
    for R, A in ((1, 1), (30, 6), (32, 32)):
        # centroids double [R,A,2], sums uint64 [R,A,3], candidates float32 [R,A,2], init int32 [R,A]; fit sums uint64 [R,3]; 8 of padding
        assert L.yf_anchor_kmeans_work_bytes(R, A) == R * A * (16 + 24 + 8 + 4) + R * 24 + 8
    assert L.yf_anchor_kmeans_work_bytes(33, 32) == 0 and L.yf_anchor_kmeans_work_bytes(0, 6) == 0


def _buf(n=4096):
    b = ctypes.create_string_buffer(n)
    return b, ctypes.addressof(b)


def test_every_refusal_comes_back_invalid_without_a_gpu():
    L = _lib.lib()
    INV = _lib.YF_E_INVALID
    keep, p = _buf()
    k0 = np.full((6, 2), 10.0)
    v = np.ones((3, 6, 2))
    s = np.array([1.0, 1.0])
    init = np.zeros((2, 6), np.int32)
    out = np.zeros(64, np.float64)
    i32 = np.zeros(64, np.int32)

    def metric(d_wh=p, n=10, d_k=p, S=1, A=6, thr=4.0, d_out=p):
        return L.yf_anchor_metric(0, d_wh, n, d_k, S, A, thr, d_out, None)

    def evolve(d_wh=p, n=10, k0=k0, v=v, A=6, gen=3, thr=4.0, work=p, wb=1 << 20, k_out=out.ctypes.data, fit=p):
        return L.yf_anchor_evolve(0, d_wh, n, None if k0 is None else k0.ctypes.data, None if v is None else v.ctypes.data, A, gen, thr, work, wb,
                                  k_out, fit, None, None)

    def kmeans(d_q=p, n=10, s=s, init=init, R=2, A=6, max_iter=100, thr=4.0, d_wh=p, work=p, wb=1 << 20):
        return L.yf_anchor_kmeans(0, d_q, n, None if s is None else s.ctypes.data, None if init is None else init.ctypes.data, R, A, max_iter, thr,
                                  d_wh, work, wb, out.ctypes.data, i32.ctypes.data, i32[8:].ctypes.data, None)

    for fn in (metric, evolve, kmeans):
        assert fn(n=0) == INV and fn(A=0) == INV and fn(A=33) == INV
        for thr in (0.5, 256.5, float("nan"), float("inf"), -4.0):
            assert fn(thr=thr) == INV, (fn.__name__, thr)
        assert fn(d_wh=None) == INV
    assert b"thr" in L.yf_last_error_string() or b"null" in L.yf_last_error_string()
    assert metric(d_k=None) == INV and metric(d_out=None) == INV and metric(S=0) == INV
    assert metric(S=171, A=6) == INV and metric(S=33, A=32) == INV                    # S * A > 1024
    assert evolve(k0=None) == INV and evolve(v=None) == INV and evolve(work=None) == INV and evolve(k_out=None) == INV and evolve(fit=None) == INV
    assert evolve(gen=0) == INV
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        kb = k0.copy()
        kb[3, 1] = bad
        assert evolve(k0=kb) == INV, bad
    vb = v.copy()
    vb[2, 5, 0] = float("nan")
    assert evolve(v=vb) == INV
    assert evolve(wb=L.yf_anchor_evolve_work_bytes(6) - 1) == _lib.YF_E_WORKSPACE
    assert kmeans(d_q=None) == INV and kmeans(s=None) == INV and kmeans(init=None) == INV and kmeans(work=None) == INV
    assert kmeans(R=0) == INV and kmeans(R=171) == INV and kmeans(max_iter=0) == INV
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert kmeans(s=np.array([1.0, bad])) == INV
    ib = init.copy()
    ib[1, 2] = 10
    assert kmeans(init=ib) == INV                                                          # row n
    ib[1, 2] = -1
    assert kmeans(init=ib) == INV
    assert kmeans(wb=L.yf_anchor_kmeans_work_bytes(2, 6) - 1) == _lib.YF_E_WORKSPACE
    del keep


def test_host_check_refuses_bad_labels_and_anchors():
    """Device arrays cannot be inspected without a synchronisation: the value rules are yf_anchor_check_host's, on host copies."""
    L = _lib.lib()

    def check(wh, k=None):
        wh = np.ascontiguousarray(wh, np.float32).reshape(-1, 2)
        k = None if k is None else np.ascontiguousarray(k, np.float32).reshape(-1, 2)
        return L.yf_anchor_check_host(wh.ctypes.data, len(wh), None if k is None else k.ctypes.data, 0 if k is None else len(k))

    good = anchor_cases.metric_labels(65)
    assert check(good) == 0 and check(good, anchor_cases.anchor_sets(2, 6)) == 0
    assert check([[0.0, 5.0]]) == 0                                  # zero is legal
    assert check([[np.float32(32768.0) - np.float32(0.002), 5.0]]) == 0
    for bad in (-1.0, -0.0 - 1e-30, float("nan"), float("inf"), 32768.0, 1e9):
        wh = good.copy()
        wh[40, 1] = bad
        assert check(wh) == _lib.YF_E_INVALID, bad
    assert b"label 40" in L.yf_last_error_string()
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        k = anchor_cases.anchor_sets(1, 6)[0].copy()
        k[4, 0] = bad
        assert check(good, k) == _lib.YF_E_INVALID, bad
    assert b"anchor 4" in L.yf_last_error_string()
    assert L.yf_anchor_check_host(None, 3, None, 0) == _lib.YF_E_INVALID
    with pytest.raises(_lib.YFError):
        aa._check_host([[1.0, -1.0]])
