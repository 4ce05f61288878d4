"""The cases of tests/val_cases.py do what they name -- checked with the oracle alone (oracle/val_oracle.py), so that no comparison in
tests/test_gpu_val_nms.py passes vacuously: the forced pass counts are the counts, the tie cases have ties inside a class, the ladder
cases suppress something and keep something, the threshold pairs evaluate in fp32 to the threshold and its two neighbours, the infinite
boxes produce NaN IoUs in the reference's own arithmetic, the overflow frame overflows."""
import numpy as np
import pytest
import torch

from oracle import val_oracle as vo
from tests import val_cases as vc

F32 = np.float32


def _count(d):
    return 0 if d is None else d.shape[0]


def _passing(case, f):
    return int((case.pred[f, :, 4] >= case.conf_thres).sum())      # torch's own comparison, as val_oracle.py:67 makes it


@pytest.mark.parametrize("group", list(vc.GROUPS))
def test_forced_pass_counts_are_the_counts(group):
    forced = 0
    for c in vc.cases(group):
        assert c.pred.dtype == torch.float32 and c.pred.dim() == 3 and c.pred.shape[2] == 5 + c.C
        if c.K is None:
            continue
        forced += 1
        assert len(c.K) == c.pred.shape[0]
        for f, K in enumerate(c.K):
            assert _passing(c, f) == K, (c.name, f)
            assert (_count(vc.reference(c)[f]) == 0) == (K == 0), (c.name, f)
    if group in ("pass_1200", "pass_4800", "ties", "thresholds", "ragged", "overflow"):
        assert forced == len(vc.cases(group))


def test_ladders_cover_the_sizes_and_counts_the_kernel_branches_on():
    sizes = [c.pred.shape[1] for c in vc.cases("size_small") + vc.cases("size_large")]
    assert sizes == [1, 63, 64, 65, 255, 256, 257, 1200, 4096, 4097, 4800, 8191]
    assert all(c.pred.shape[0] == 2 and c.C == 3 for c in vc.cases("size_small") + vc.cases("size_large"))
    for M in (1200, 4800):
        got = vc.cases("pass_%d" % M)
        assert [c.name.split("_", 2)[2] for c in got] == list(vc.PLACEMENTS)
        for c in got:
            assert c.K == [0, 1, 64, 65, 256, 257, 1024, 1025, M]
            for f, K in enumerate(c.K):
                rows = np.nonzero(c.pred[f, :, 4].numpy() >= F32(0.5))[0]
                trips = [((rows >= b) & (rows < b + vc.POST_THREADS)).sum() for b in range(0, M, vc.POST_THREADS)]
                if c.name.endswith("first_trip") and K:
                    assert rows[0] == 0 and rows[-1] == K - 1
                    assert trips[0] == min(K, 1024) and (K > 1024 or trips[-1] == 0)      # a trip that passes whole, trips that pass nothing
                if c.name.endswith("last_trip") and K:
                    assert rows[-1] == M - 1 and rows[0] == M - K
                    assert trips[-1] == min(K, M % 1024) and (K >= M - 1024 or trips[0] == 0)
    assert [c.C for c in vc.cases("argmax")] == [1, 2, 3, 20, 80]
    assert vc.cases("ragged")[0].K == [900, 0, 1, 0, 1200]


@pytest.mark.parametrize("group", ["size_small", "size_large", "pass_1200", "pass_4800", "argmax", "ragged"])
def test_ladder_cases_suppress_and_keep(group):
    for c in vc.cases(group):
        ref = vc.reference(c)
        for f in range(c.pred.shape[0]):
            K = _passing(c, f)
            if c.flags.get("degenerate") or K < 64:
                assert _count(ref[f]) == min(K, _count(ref[f])) and (K == 0) == (ref[f] is None)
                continue
            assert 1 <= _count(ref[f]) < K, (c.name, f, K)


def test_tie_cases_hold_ties_inside_a_class():
    for c in vc.cases("ties"):
        assert len(np.unique(c.pred[..., 4].numpy())) == 7
        for f in range(2):
            p = c.pred[f]
            keep = p[:, 4] >= c.conf_thres
            cls = p[:, 5:].max(1).indices[keep].numpy()
            conf = p[keep, 4].numpy()
            rows = np.nonzero(keep.numpy())[0]
            pairs, straddle = 0, 0
            for k in range(c.C):
                _, n = np.unique(conf[cls == k], return_counts=True)
                pairs += int((n * (n - 1) // 2).sum())
            assert pairs >= 200, (c.name, f, pairs)
            # equal confidences in neighbouring rows of different classes, and a run of one value longer than a wave
            straddle = int(((conf[1:] == conf[:-1]) & (cls[1:] != cls[:-1]) & (rows[1:] == rows[:-1] + 1)).sum())
            assert straddle >= 10
            assert (p[100:200, 4] == p[100, 4]).all() and p[100, 4] >= c.conf_thres
            assert 1 <= _count(vc.reference(c)[f]) < int(keep.sum())
    ident = vc.cases("ties")[1]
    p = ident.pred[0]
    same = (p[:, 4] == p[100, 4])
    assert (p[same][:, :4] == p[100, :4]).all()


def test_argmax_cases_have_tied_class_scores():
    """the expected class is what torch.max returns on this host: the first maximum"""
    for c in vc.cases("argmax"):
        if c.C == 1:
            continue
        tied, first = 0, 0
        for f in range(2):
            s = c.pred[f, :, 5:]
            mx = s.max(1)
            n = (s == mx.values[:, None]).sum(1)
            tied += int((n >= 2).sum())
            firstmax = (s == mx.values[:, None]).float().argmax(1)
            assert torch.equal(firstmax, mx.indices)
            first += int(((n >= 2) & (c.pred[f, :, 4] >= 0.5)).sum())
        assert tied >= 240 and first >= 60, (c.name, tied, first)


def test_conf_threshold_rows_sit_on_the_threshold_and_its_neighbours():
    got = vc.cases("thresholds")[:3]
    assert [c.conf_thres for c in got] == [0.5, 0.7, 0.3]
    for c in got:
        t = F32(c.conf_thres)
        conf = c.pred[..., 4].numpy()
        for f in range(2):
            at, below, above = (conf[f] == t).sum(), (conf[f] == np.nextafter(t, F32(0))).sum(), (conf[f] == np.nextafter(t, F32(1))).sum()
            assert (at, below, above) == (10, 10, 10)
            # torch compares in float32: the rows AT float32(thres) pass, the rows below do not (in double, float32(0.7) < 0.7 would fail)
            mask = c.pred[f, :, 4] >= c.conf_thres
            assert bool(mask[conf[f] == t].all()) and not bool(mask[conf[f] == np.nextafter(t, F32(0))].any())
    assert float(F32(0.7)) < 0.7 and float(F32(0.3)) > 0.3


def test_iou_pairs_evaluate_to_the_threshold_and_its_neighbours():
    got = vc.cases("thresholds")[3:]
    assert [c.nms_thres for c in got] == [0.25, 0.5]
    for c in got:
        t = F32(c.nms_thres)
        want = {"equal": t, "below": np.nextafter(t, F32(0)), "above": np.nextafter(t, F32(1))}
        for kind, (W1, H1, W2, H2) in vc.IOU_PAIRS[c.nms_thres].items():
            for ox, oy in ((0, 0), (110000, 20000)):
                rows = torch.from_numpy(np.stack([vc._corner_row(ox, oy, W1, H1, 0.9), vc._corner_row(ox, oy, W2, H2, 0.6)]))
                corners = torch.stack([rows[:, 0] - rows[:, 2] / 2, rows[:, 1] - rows[:, 3] / 2, rows[:, 0] + rows[:, 2] / 2,
                                       rows[:, 1] + rows[:, 3] / 2], 1)
                assert corners.tolist() == [[ox, oy, ox + W1 - 1, oy + H1 - 1], [ox, oy, ox + W2 - 1, oy + H2 - 1]]
                iou = vo.bbox_iou(corners[:1], corners[1:])
                assert iou.dtype == torch.float32 and iou.numpy()[0] == want[kind], (c.nms_thres, kind, float(iou))
        ref = vc.reference(c)
        for f in range(2):
            assert _count(ref[f]) == c.flags["survivors"][f] == 16      # 12 first boxes + the 4 partners below the threshold


def _trace(case, f):
    """val_oracle.non_max_suppression for one frame, step by step with its own bbox_iou: -> (detections, number of NaN IoUs)"""
    p = case.pred[f].clone()
    c = p.clone()
    c[:, 0], c[:, 1] = p[:, 0] - p[:, 2] / 2, p[:, 1] - p[:, 3] / 2
    c[:, 2], c[:, 3] = p[:, 0] + p[:, 2] / 2, p[:, 1] + p[:, 3] / 2
    c = c[c[:, 4] >= case.conf_thres]
    conf, pred = torch.max(c[:, 5:], 1, keepdim=True)
    det = torch.cat((c[:, :5], conf, pred.float()), 1)
    out, nans = [], 0
    for cl in det[:, -1].unique():
        dc = det[det[:, 6] == cl]
        dc = dc[torch.sort(dc[:, 4], descending=True, stable=True)[1]]
        while dc.size(0):
            out.append(dc[0])
            if len(dc) == 1:
                break
            ious = vo.bbox_iou(dc[:1], dc[1:])
            nans += int(torch.isnan(ious).sum())
            dc = dc[1:][ious < case.nms_thres]
    return torch.stack(out), nans


def test_infinite_boxes_give_nan_ious_in_the_oracle():
    (c,) = vc.cases("degenerate")
    ref = vc.reference(c)
    for f in range(2):
        det, nans = _trace(c, f)
        assert torch.equal(det, ref[f])                       # the trace is the oracle
        assert nans >= 1, f
        p = c.pred[f]
        assert int(torch.isinf(p[:, 2]).sum()) == 24 and int(torch.isinf(p[:, 3]).sum()) == 24
        assert int(((p[:, 2] == 0) | (p[:, 3] == 0)).sum()) == 24 and int((p[:, 2] > 1e5).sum()) >= 36
        assert bool(torch.isinf(ref[f][:, :4]).any())         # infinite corners reach the output rows
        inf_conf = p[torch.isinf(p[:, 2]) | torch.isinf(p[:, 3]), 4]
        rest = p[~(torch.isinf(p[:, 2]) | torch.isinf(p[:, 3])), 4]
        assert (inf_conf.min() > rest.max()) if f == 0 else (inf_conf.max() < rest[rest >= 0.5].min())
    # the suppressor of frame 0's first class is infinite; frame 1's is not
    assert bool(torch.isinf(ref[0][0, :4]).any()) and not bool(torch.isinf(ref[1][0, :4]).any())


def test_overflow_frame_has_more_survivors_than_kmax():
    (c,) = vc.cases("overflow")
    n = [_count(d) for d in vc.reference(c)]
    assert n[1] > vc.OVERFLOW_KMAX and 0 < n[0] <= vc.OVERFLOW_KMAX and n[2] == 0, n


def test_decode_inputs_and_the_float64_reference():
    """the planted logits are there, and the float64 formulae agree with val_oracle.decode_head to fp32 rounding where nothing saturates"""
    anchors = [[12, 18], [37, 49], [52, 132]]
    x, planted = vc.decode_head(1, 3, 3, 3, 8, 10)
    assert x.shape == (3, 24, 8, 10) and x.dtype == np.float32
    for v in vc.PLANTED_LOGITS:
        hit = (x == v) & planted & (np.signbit(x) == np.signbit(v))
        assert hit.reshape(3, 3, 8, 80).any(3).all(), v                 # every planted value in every channel kind
    got = vo.decode_head(torch.from_numpy(x), anchors, 3, [256, 320]).numpy()
    want = vc.decode_f64(x, anchors, 3, 256, 320)
    err = vc.ulp_error(got, want)
    with np.errstate(over="ignore"):
        w32 = want.astype(np.float32)
    assert np.isinf(w32).any() and np.array_equal(np.isinf(w32), np.isinf(got))
    assert (want[..., 4:] == 1.0).any()                                 # sigmoid(87), sigmoid(100) are 1 in float64 too
    bulk = ~planted.reshape(3, 3, 8, 8, 10).transpose(0, 1, 3, 4, 2).reshape(want.shape)
    assert np.nanmax(err[bulk]) <= 8, np.nanmax(err[bulk])              # same formulae: a few roundings apart
    assert vc.ulp_error(np.float32([1.0, 0.0, 1e-45]), np.float64([1.0 + 2.0 ** -23, 2.0 ** -149, 0.0])).tolist() == [1.0, 1.0, 1.0]
