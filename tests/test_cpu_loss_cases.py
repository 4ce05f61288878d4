"""The oracle side of the training-loss tests (tests/loss_cases.py; the kernels are held to it in tests/test_gpu_loss.py), without a GPU:

  * oracle/loss_oracle.py::loss_model64 is pinned: with the sigmoid left in float64 (round_p=False) its seven losses and its analytic
    gradient equal torch autograd of loss_head run in float64 to 1e-12 relative, on every case of logit set M (|logit| <= 12);
  * every case of the table has the property it names, asserted on the oracle's own fp32 values;
  * the fp32 twin (loss_head in float32 with autograd) stays inside the table's condition on every case of sets M and S;
  * every planted defect is rejected by the comparator on at least one case.

PLANTED DEFECTS and the rule the suite had before (test_gpu_parity.py's random trials: the seven losses to rtol 3e-5, the gradient to
max|g - g_ref| <= 3e-5 max|g_ref| over the whole tensor, skipped without a positive cell).  "Old rule" = that rule applied to THIS case
table; the test prints the table below.  The old rule does reject the five target defects on these cases: at these sizes one wrong cell
moves a sum by far more than 3e-5 -- what the old suite lacked there was the cases (no tie, no box on the threshold, no two targets of
one anchor in a cell), and the planes are now compared directly.  What the old RULE lets through is in the last column:
  defect                                   rejected here on                                    of these, accepted by the old rule
  last-maximum argmax                      tie_same, tie_swap, small, small_S                  -
  >= at the ignore threshold               thres, thres_S                                      -
  the contracted IoU                       thres, thres_S                                      -
  a one-hot that overwrites                cell_same, cell_same_S and 11 more                  -
  tx taken from a cell's first target      cell_same, cell_same_S and 13 more                  -
  cls / n_pos without C                    all 27 judged cases with C > 1 and a positive cell  -
  the x gradient without the mask factor   all 32 judged cases                                 nopos, nopos_S, e3_S
  the no-object conf gradient x 1.02       all 32 judged cases                                 nopos, nopos_S, n65_S, small_S, thres_S,
                                                                                               cell_same_S, a8c20_S, and the issue's
                                                                                               example: batch 16 on the stride-16 head
The old rule never looked at the gradient of a batch without a positive cell (nopos), and wherever a few elements are much larger than
the rest -- class gradients of few positives at batch 16, box gradients of saturated logits in set S -- a relative error of 2 % in every
no-object confidence gradient disappears under 3e-5 of the largest element.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_cases as lc  # noqa: E402
from oracle import loss_oracle as lo  # noqa: E402

CASES = lc.cases()
BY = {c.name: c for c in CASES}
JUDGED = [c for c in CASES if c.logit_set != "band"]


def _anchors(c):
    return lo.scaled_anchors(c.anchors, (c.H, c.W), c.fh, c.fw)


# ---- the model ----

@pytest.mark.parametrize("case", [c for c in CASES if c.logit_set == "M"], ids=lambda c: c.name)
def test_model64_equals_float64_autograd_of_loss_head(case):
    """Everything in float64 (default dtype float64 while loss_head runs: its planes hold the same float32 tx, ty and the unrounded log for
    tw, th, and are handed to the model).  1e-12 of each loss, 1e-12 of the gradient's largest element per kind."""
    ref = lc.reference(case)
    x = torch.from_numpy(case.logits).double().requires_grad_(True)
    assert float(x.abs().max()) <= 12
    torch.set_default_dtype(torch.float64)
    try:
        planes = lo.get_target(ref["clean"], _anchors(case), case.fw, case.fh, lc.THRES, case.C)
        out = lo.loss_head(x, ref["clean"], case.anchors, case.C, (case.H, case.W), lc.THRES)
        out[0].backward()
    finally:
        torch.set_default_dtype(torch.float32)
    assert planes[0].dtype == torch.float64 and torch.equal(planes[0].float(), ref["planes"][0]) and torch.equal(planes[2].float(), ref["planes"][2])
    m = lo.loss_model64(case.logits, ref["clean"], case.anchors, case.C, (case.H, case.W), lc.THRES, planes=planes, round_p=False)
    want = np.array([out[0].item()] + list(out[1:]))
    for i, name in enumerate(lo.LOSS_NAMES):
        if math.isnan(want[i]):
            assert math.isnan(m["losses"][i]) and ref["m64"]["n_pos"] == 0 and name in ("total", "cls")
        else:
            assert abs(m["losses"][i] - want[i]) <= 1e-12 * abs(want[i]), (name, m["losses"][i], want[i])
    g = x.grad.numpy().reshape(ref["kinds"]["x"].shape)
    mg = m["grad"].reshape(g.shape)
    assert np.isfinite(g).all()
    for name, sel in ref["kinds"].items():
        if sel.any():
            assert np.abs(mg[sel] - g[sel]).max() <= 1e-12 * np.abs(g[sel]).max(), name
            if name in ("box_off", "conf_ignored", "cls_off"):
                assert (g[sel] == 0).all() and (mg[sel] == 0).all()


def test_the_rounded_sigmoid_is_what_separates_the_model_from_plain_float64():
    """logit 20: float32(sigmoid) is 1, log(1 - p) the clamp -100 and the gradient 0; plain float64 gives 20.0 and p / E.  And torch's own
    float32 sigmoid is within SIGMOID_ULPS float32 steps of the correctly rounded one on [-12, 12] (the twin condition's allowance)."""
    x = np.full((1, 6, 1, 1), 20.0, np.float32)
    t = torch.zeros(1, 1, 6)
    a = lo.loss_model64(x, t, [[16, 16]], 1, (16, 16))
    b = lo.loss_model64(x, t, [[16, 16]], 1, (16, 16), round_p=False)
    assert a["terms"]["conf_noobj"].item() == 100.0 and a["grad"][0, 4, 0, 0] == 0.0
    assert abs(b["terms"]["conf_noobj"].item() - 20.0) < 1e-6 and abs(b["grad"][0, 4, 0, 0] - 0.5) < 1e-8
    v = np.linspace(-12, 12, 400001).astype(np.float32)
    got = torch.sigmoid(torch.from_numpy(v)).numpy().view(np.int32).astype(np.int64)
    want = (1.0 / (1.0 + np.exp(-v.astype(np.float64)))).astype(np.float32).view(np.int32)
    assert np.abs(got - want).max() <= lc.SIGMOID_ULPS


# ---- the table ----

def test_the_table_covers_the_listed_geometry():
    E = {c.N * c.A * c.fh * c.fw for c in CASES}
    assert {3, 15, 16, 17, 255, 256, 257} <= E
    for n in ("e255", "e256", "e257"):
        assert BY[n].A == 1 and BY[n].N == 1
    assert {(1, 1), (3, 5), (4, 6), (8, 10), (16, 20), (15, 17), (16, 16), (1, 257)} <= {(c.fh, c.fw) for c in CASES}
    assert {1, 2, 64, 65, 130} <= {c.N for c in CASES}
    assert {1, 2, 3, 8} <= {c.A for c in CASES} and {1, 3, 5, 20} <= {c.C for c in CASES} and {1, 3, 50} <= {c.T for c in CASES}
    assert any(c.H * c.fw != c.W * c.fh for c in CASES)
    assert any((c.fh * c.fw) % 2 for c in CASES)
    assert len({c.name for c in CASES}) == len(CASES)
    for c in CASES:
        assert c.targets.shape == (c.N, c.T, 6) and c.logits.shape == (c.N, c.A * (5 + c.C), c.fh, c.fw)
        assert c.targets.dtype == np.float32 and c.logits.dtype == np.float32 and c.counted == lc.reference(c)["counted"]


@pytest.mark.parametrize("case", [c for c in CASES if c.logit_set == "M"], ids=lambda c: c.name)
def test_numpy_get_target_is_the_oracles_bit_for_bit(case):
    """tests/loss_cases.py::get_target_np (which carries the planted target defects) and iou32 (which the threshold search runs on)"""
    ref = lc.reference(case)
    got = lc.get_target_np(ref["clean"].numpy(), lc.anchors32(case), case.fw, case.fh, case.C)
    for name, a, b in zip(("mask", "noobj", "tx", "ty", "tw", "th", "tcls"), got, ref["planes"]):
        assert a.dtype == b.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32)), name


def test_threshold_targets_sit_on_the_threshold_in_the_oracles_own_arithmetic():
    c, rows = BY["thres"], lc.threshold_rows()
    ref = lc.reference(c)
    anc = _anchors(c)
    anchor_shapes = torch.FloatTensor(np.concatenate((np.zeros((3, 2)), np.array(anc)), 1))
    t32 = np.float32(lc.THRES)
    want = {"exact": t32, "below": np.nextafter(t32, np.float32(0)), "above": np.nextafter(t32, np.float32(1))}
    n = {"exact": 0, "below": 0, "above": 0, "flips": 0}
    noobj, mask = ref["planes"][1].numpy(), ref["planes"][0].numpy()
    for i, (kind, w, h, a, flips) in enumerate(rows):
        b, j = divmod(i, c.T)
        tgt = torch.from_numpy(c.targets[b, j])
        assert tgt[2].item() == np.float32(w) and tgt[3].item() == np.float32(h)
        gw, gh = tgt[2] * c.fw, tgt[3] * c.fh
        iou = lo._bbox_iou(torch.FloatTensor(np.array([0.0, 0.0, gw, gh], dtype=np.float32)).unsqueeze(0), anchor_shapes).numpy()
        mine = lc.iou32(gw.numpy(), gh.numpy(), lc.anchors32(c)[:, 0], lc.anchors32(c)[:, 1])
        assert np.array_equal(iou.view(np.int32), mine.view(np.int32))
        assert iou[a] == want[kind], (kind, iou[a])
        n[kind] += 1
        gi, gj = int(tgt[0] * c.fw), int(tgt[1] * c.fh)
        assert mask[b, :, gj, gi].sum() == 1                                   # its own cell
        assert noobj[b, a, gj, gi] == (0.0 if kind == "above" else 1.0)        # > , not >=
        con = lc.iou32(gw.numpy(), gh.numpy(), lc.anchors32(c)[:, 0], lc.anchors32(c)[:, 1], contracted=True)
        assert bool((con[a] > t32) != (iou[a] > t32)) == flips
        n["flips"] += kind == "exact" and flips
    assert n["exact"] >= 32 and n["below"] >= 32 and n["above"] >= 32 and n["flips"] >= 16, n
    assert BY["thres_S"].targets is c.targets


def test_tie_collision_edge_and_skip_cases_do_what_they_name():
    # identical anchors: both IoUs equal and maximal somewhere, anchor 1 never positive
    for name in ("tie_same", "tie_swap"):
        c = BY[name]
        ref = lc.reference(c)
        a32 = lc.anchors32(c)
        tied = 0
        for b in range(c.N):
            for t in c.targets[b]:
                iou = lc.iou32(t[2] * np.float32(c.fw), t[3] * np.float32(c.fh), a32[:, 0], a32[:, 1])
                assert iou[0] == iou[1]
                tied += iou[0] >= iou[2]
        m = ref["planes"][0].numpy()
        assert tied >= 3 and m[:, 1].sum() == 0 and m[:, 0].sum() >= 3, (name, tied)
    assert BY["tie_swap"].H * BY["tie_swap"].fw == BY["tie_swap"].W * BY["tie_swap"].fh
    # four targets, one cell, one anchor
    c = BY["cell_same"]
    m, _, tx, ty, tw, th, tcls = (p.numpy() for p in lc.reference(c)["planes"])
    for b in range(c.N):
        assert m[b].sum() == 2 and m[b, :, 1, 2].sum() == 1
        a = int(np.argmax(m[b, :, 1, 2]))
        assert tcls[b, a, 1, 2].tolist() == [1.0, 1.0, 1.0]                     # accumulated over classes 0, 1, 2, 0
        last = c.targets[b, 3]
        assert tx[b, a, 1, 2] == last[0] * np.float32(6) - 2 and ty[b, a, 1, 2] == last[1] * np.float32(4) - 1
        assert tx[b, a, 1, 2] != c.targets[b, 0, 0] * np.float32(6) - 2
    # four targets, one cell, three anchors
    c = BY["cell_diff"]
    m, noobj = (p.numpy() for p in lc.reference(c)["planes"][:2])
    assert m[0, :, 2, 3].tolist() == [1.0, 1.0, 1.0] and m.sum() == 3
    assert lc.reference(c)["planes"][6].numpy()[0, 1, 2, 3].tolist() == [1.0, 1.0, 0.0]   # anchor 1 was best twice: classes 1 and 0
    # integral and last-cell coordinates
    c = BY["edges"]
    m, _, tx, ty = (p.numpy() for p in lc.reference(c)["planes"][:4])
    for k, gi in enumerate((0, 1, 7, 15)):
        gj = (gi * 5) % 16
        assert m[0, :, gj, gi].sum() == 1 and tx[0, :, gj, gi].sum() == 0 and ty[0, :, gj, gi].sum() == 0
    for k, e in enumerate((1, 2, 5, 10, 15, 19)):
        a = int(np.argmax(m[0, :, 15, 15]))
        assert c.targets[0, 4 + k, 0] * np.float32(16) == np.float32(16 - 2.0 ** -e) and m[0, a, 15, 15] == 1
    assert tx[0, int(np.argmax(m[0, :, 15, 15])), 15, 15] == np.float32(1 - 2.0 ** -19)    # the last of the six
    assert m[1, :, 15, 15].sum() == 1 and c.targets[1, 0, 0] < 1 and lc.reference(c)["counted"] == 0
    # x < k / fw in exact arithmetic, float32(x * fw) == k
    c = BY["roundup"]
    m, _, tx = (p.numpy() for p in lc.reference(c)["planes"][:3])
    ups = lc.interior_roundups(20)
    for k, (xn, col) in enumerate(ups[:6]):
        assert float(np.float32(xn)) * 20 < col and (torch.tensor(xn) * 20).item() == col
        assert m[0, :, k, col].sum() == 1 and m[0, :, k, col - 1].sum() == 0 and tx[0, :, k, col].sum() == 0
    for fw in (3, 5, 6, 10, 17, 20, 257):                                       # and never up to fw itself
        assert (torch.tensor(float(np.nextafter(np.float32(1), np.float32(0)))) * fw).item() < fw
    assert m[0, :, 8, 19].sum() == 1
    # skipped sizes
    c = BY["skipped"]
    m = lc.reference(c)["planes"][0].numpy()
    assert m.sum() == 1 and m[0, :, 1, 1].sum() == 1 and lc.reference(c)["planes"][6].numpy()[0, :, 1, 1].sum(0).tolist() == [0.0, 0.0, 1.0]
    # class ids
    c = BY["cls_trunc"]
    tc = lc.reference(c)["planes"][6].numpy()
    assert tc[0, :, 0, 1].sum(0).tolist() == [0.0, 0.0, 1.0] and tc[0, :, 2, 3].sum(0).tolist() == [1.0, 0.0, 0.0]


def test_counted_targets_are_the_ones_the_reference_cannot_index():
    c = BY["counted"]
    ref = lc.reference(c)
    assert ref["counted"] == 5 and ref["m64"]["n_pos"] == 3
    anc = _anchors(c)
    with pytest.raises(IndexError):                                             # class == C: yolo_loss.py:195
        lo.get_target(torch.from_numpy(c.targets[0:1]), anc, c.fw, c.fh, lc.THRES, c.C)
    with pytest.raises(IndexError):                                             # column fw, row fh + 1
        lo.get_target(torch.from_numpy(c.targets[2:3, 1:]), anc, c.fw, c.fh, lc.THRES, c.C)
    # the reference wraps negative indices round; this project counts them (include/yolo_fastest_hip.h)
    wrap_cls = lo.get_target(torch.from_numpy(c.targets[1:2, :1]), anc, c.fw, c.fh, lc.THRES, c.C)
    assert wrap_cls[6][0, :, 0, 1].sum(0).tolist() == [0.0, 0.0, 1.0]
    wrap_col = lo.get_target(torch.from_numpy(c.targets[2:3, :1]), anc, c.fw, c.fh, lc.THRES, c.C)
    assert wrap_col[0][0, :, 2, 5].sum() == 1
    assert ref["planes"][0][1].sum() == 1 and ref["planes"][0][2].sum() == 1 and ref["planes"][0][2, :, 2, 5].sum() == 0
    for other in CASES:
        assert (other.counted > 0) == (other.name == "counted")


def test_empty_images_end_markers_and_the_batch_without_targets():
    c = BY["n64"]
    m = lc.reference(c)["planes"][0].numpy()
    assert m[5].sum() == 0 and m[63].sum() == 0 and m[7].sum() == 0 and m[9].sum() == 1 and m[6].sum() >= 1
    assert c.targets[7, 1, 5] == 255.0 and c.targets[7, 0, 5] == 0
    m = lc.reference(BY["n130"])["planes"][0].numpy()
    assert m[64].sum() == 0 and m[129].sum() == 1 and m[65:129].sum() > 64
    for name in ("nopos", "nopos_S"):
        ref = lc.reference(BY[name])
        assert ref["m64"]["n_pos"] == 0 and ref["planes"][1].min() == 1
        assert np.isnan(ref["m64"]["losses"][[0, 6]]).all() and np.isfinite(ref["m64"]["losses"][1:6]).all()
        assert np.isnan(ref["twin_losses"][[0, 6]]).all() and np.isfinite(ref["twin_grad"]).all()
        assert np.abs(ref["m64"]["grad"]).max() > 0


def test_logit_sets():
    seen = {k: set() for k in ("conf_pos", "conf_noobj", "conf_ignored", "x", "cls")}
    for c in CASES:
        x = c.logits
        if c.logit_set == "M":
            assert np.abs(x).max() <= 12
        elif c.logit_set == "S":
            big = np.abs(x) > 12
            assert set(np.unique(x[big]).tolist()) <= set(lc.S_VALUES.tolist()) and big.any() and not big.all()
            assert x.size < 1000 or 0.45 < big.mean() < 0.55
            assert not (((x > 15) & (x < 18)) | ((x > -105) & (x < -86))).any()
            kinds = lc.reference(c)["kinds"]
            xr = x.reshape(kinds["x"].shape)
            for k in seen:
                seen[k] |= set(np.unique(xr[kinds[k] & (np.abs(xr) > 12)]).tolist())
        else:
            assert (((x > 15) & (x < 18)) | ((x > -105) & (x < -86))).all()
    for k, vals in seen.items():                                                # positive, no-object and ignored cells alike
        assert vals == set(lc.S_VALUES.tolist()), (k, sorted(vals))
    assert sum(c.logit_set == "band" for c in CASES) == 2


# ---- the twin ----

@pytest.mark.parametrize("case", JUDGED, ids=lambda c: c.name)
def test_the_twin_is_within_the_tables_condition_and_passes_the_comparator(case, capsys):
    ref = lc.reference(case)
    assert lc.twin_condition(case) == []
    l8 = np.append(ref["twin_losses"], np.float32(ref["counted"]))
    rep = lc.judge(case, l8, ref["twin_grad"], lc.planes_to_dense(ref["planes"]))
    assert rep.ok and rep.plane_diffs == 0, rep.failures
    bad = lc.judge(case, np.append(ref["twin_losses"], np.float32(ref["counted"] + 1)))
    assert not bad.ok


@pytest.mark.parametrize("case", [c for c in CASES if c.logit_set == "band"], ids=lambda c: c.name)
def test_band_cases_are_finite_in_the_reference(case):
    ref = lc.reference(case)
    rep = lc.judge(case, np.append(ref["twin_losses"], np.float32(0)), ref["twin_grad"], lc.planes_to_dense(ref["planes"]))
    assert rep.ok, rep.failures
    g = ref["twin_grad"].copy()
    g.reshape(-1)[3] = np.inf
    assert not lc.judge(case, np.append(ref["twin_losses"], np.float32(0)), g).ok


# ---- planted defects ----

def _old_rule(losses7, grad, ref):
    """test_gpu_parity.py::test_training_loss_matches_the_reference's random trials"""
    wl, wg = ref["twin_losses"], ref["twin_grad"]
    if not np.allclose(np.asarray(losses7, np.float32), wl, rtol=3e-5, atol=1e-7, equal_nan=True):
        return False
    return (not np.isfinite(wl[0])) or bool(np.abs(np.asarray(grad, np.float64).reshape(wg.shape) - wg).max() <= 3e-5 * np.abs(wg).max() + 1e-10)


def _grad_defect(case, which):
    ref = lc.reference(case)
    shape = ref["kinds"]["x"].shape
    g = ref["twin_grad"].astype(np.float64).reshape(shape).copy()
    if which == "cls_without_C":
        g[:, :, 5:] *= case.C
    elif which == "x_without_mask":
        with np.errstate(over="ignore"):
            p = 1.0 / (1.0 + np.exp(-case.logits.reshape(shape)[:, :, 0].astype(np.float64)))
        m, tx = ref["planes"][0].numpy(), ref["planes"][2].numpy()
        g[:, :, 0] = 2.5 / m.size * (p - tx * m)
    elif which == "noobj_x_1.02":
        g[ref["kinds"]["conf_noobj"]] *= 1.02
    return g.astype(np.float32).reshape(case.logits.shape)


DEFECTS_GRAD = ("cls_without_C", "x_without_mask", "noobj_x_1.02")


def _batch16_large_head():
    """the issue's example: the shipped stride-16 head at the reference's batch 16, eight images with one target each"""
    rng = np.random.default_rng(16)
    t = np.zeros((16, 1, 6), np.float32)
    t[::2, 0] = np.concatenate([rng.uniform(0.1, 0.9, (8, 2)), rng.uniform(0.05, 0.3, (8, 2)), rng.integers(0, 3, (8, 1)), np.full((8, 1), 255.0)], 1)
    x = np.clip(rng.normal(0, 3, (16, 24, 16, 20)), -12, 12).astype(np.float32)
    return lc.Case("batch16", 16, 3, 3, 16, 20, 256, 320, 1, lc.ANC_LARGE, t, x, "", "M", 0)


def test_every_planted_defect_is_rejected_by_at_least_one_case(capsys):
    lines = []
    for d in lc.DEFECTS_TARGET:
        new, old = [], []
        for c in JUDGED:
            ref = lc.reference(c)
            planes = lc.get_target_np(ref["clean"].numpy(), lc.anchors32(c), c.fw, c.fh, c.C, defect=d)
            if all(torch.equal(a, b) for a, b in zip(planes, ref["planes"])):
                continue
            rep = lc.Report(c)
            lc.judge_planes(rep, lc.planes_to_dense(planes), ref["planes"])
            assert not rep.ok                                                   # any plane that differs at all is rejected
            new.append(c.name)
            m = lo.loss_model64(c.logits, ref["clean"], c.anchors, c.C, (c.H, c.W), lc.THRES, planes=planes)
            if _old_rule(m["losses"], m["grad"], ref):
                old.append(c.name)
        lines.append("  %-18s rejected on %s; of these the old rule accepts %s" % (d, new, old))
        assert new, d
    want = {"argmax_last": ("tie_same", "tie_swap"), "thres_ge": ("thres",), "iou_contracted": ("thres",), "onehot_overwrites": ("cell_same",),
            "tx_first": ("cell_same",)}
    for d, names in want.items():                                               # each defect by the case made for it
        for name in names:
            c, ref = BY[name], lc.reference(BY[name])
            planes = lc.get_target_np(ref["clean"].numpy(), lc.anchors32(c), c.fw, c.fh, c.C, defect=d)
            assert not all(torch.equal(a, b) for a, b in zip(planes, ref["planes"])), (d, name)
    for d in DEFECTS_GRAD:
        new, old = [], []
        for c in JUDGED + [_batch16_large_head()]:
            ref = lc.reference(c)
            g = _grad_defect(c, d)
            rep = lc.Report(c)
            lc.judge_grad(rep, g, ref["m64"]["grad"], ref["twin_grad"], ref["kinds"])
            if not rep.ok:
                new.append(c.name)
                if _old_rule(ref["twin_losses"], g, ref):
                    old.append(c.name)
        lines.append("  %-18s rejected on %d cases; of these the old rule accepts %s" % (d, len(new), old))
        if d == "cls_without_C":                                                # no defect with one class, no class gradient without a positive
            assert set(new) == {c.name for c in JUDGED if c.C > 1 and lc.reference(c)["m64"]["n_pos"]} | {"batch16"}
        else:
            assert set(new) == {c.name for c in JUDGED} | {"batch16"}, (d, new)
        if d == "noobj_x_1.02":                                                 # the issue's 2 % at batch 16, and the batch the old rule never looked at
            assert "batch16" in old and "nopos" in old and "nopos_S" in old
    with capsys.disabled():
        print("\n[planted defects]\n" + "\n".join(lines))
