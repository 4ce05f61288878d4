"""The definition side of yolov5's objectness / class loss options (tests/loss_hyp_ref.py; the kernels are held to it in
tests/test_gpu_loss_hyp.py), without a GPU:

  * the definition against a transcription of yolov5's smooth_BCE, FocalLoss and BCEWithLogitsLoss(pos_weight=) in float64 on logits
    |x| <= 12: the two forms differ only by the clamps (inactive there) and by log(1 - p) taken from a rounded p, at most
    2^-52 / e^-12 = 3.6e-11 per element; 1e-9 absolute is asserted;
  * the model's closed-form gradient (round_p=False) against float64 autograd of the definition, per case and option set;
  * with neutral options the model IS oracle.loss_oracle.loss_model64 / box_loss_ref's model, exactly;
  * every added case has the property it names; every judged case is finite (cls and total NaN without a positive cell); the twin alone
    stays inside `twin_condition`, and which cases its two added allowances let in is pinned;
  * the comparator rejects the eight planted defects and passes the model itself;
  * csrc/yf_loss_term.h -- the function the kernel calls per element, compiled for the host -- against float64 autograd of `element` on a
    grid of (p, t, w, gamma) that includes p = 0 and p = 1;
  * the header and _lib name the new entries; YOLOLossV3 and train() refuse what the entry refuses.
"""
import copy
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import box_loss_ref as br  # noqa: E402
import loss_cases as lc  # noqa: E402
import loss_hyp_ref as hr  # noqa: E402

JUDGED = hr.judged_cases()
SUBSET = [hr.case_by_name(n) for n in hr.SUBSET]


def _cases_of(name):
    return JUDGED if name.startswith("all") else SUBSET


# ---- yolov5, transcribed (utils/loss.py: smooth_BCE, FocalLoss; ComputeLoss builds BCEWithLogitsLoss(pos_weight=...)) ----

def _v5_smooth_bce(eps=0.1):
    return 1.0 - 0.5 * eps, 0.5 * eps


def _v5_focal(pred, true, pos_weight, gamma, alpha):
    loss = torch.nn.BCEWithLogitsLoss(pos_weight=torch.tensor([pos_weight], dtype=pred.dtype), reduction="none")(pred, true)
    if gamma > 0:
        pred_prob = torch.sigmoid(pred)
        p_t = true * pred_prob + (1 - true) * (1 - pred_prob)
        alpha_factor = true * alpha + (1 - true) * (1 - alpha)
        modulating_factor = (1.0 - p_t) ** gamma
        loss = loss * (alpha_factor * modulating_factor)
    return loss


@pytest.mark.parametrize("gamma,alpha", [(0.0, 0.25), (1.0, 0.25), (1.5, 0.25), (2.0, 0.7)])
@pytest.mark.parametrize("w", [1.0, 0.6, 2.5])
def test_the_definition_is_yolov5s(w, gamma, alpha):
    g = torch.Generator().manual_seed(11)
    x = (torch.rand(4096, generator=g, dtype=torch.float64) * 24 - 12)
    x[:4] = torch.tensor([12.0, -12.0, 0.0, 11.999])
    cp, cn = _v5_smooth_bce(0.1)
    iou = torch.rand(4096, generator=g, dtype=torch.float64)
    for t in (torch.ones_like(x), torch.zeros_like(x), torch.where(iou < 0.5, torch.full_like(x, cp), torch.full_like(x, cn)), iou):
        x1, x2 = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        want = _v5_focal(x1, t, w, gamma, alpha)
        got = hr.element(torch.sigmoid(x2), t, w, hr.opts(fl_gamma=gamma, fl_alpha=alpha))
        assert float((got - want).detach().abs().max()) <= 1e-9
        want.sum().backward()
        got.sum().backward()
        assert float((x1.grad - x2.grad).abs().max()) <= 1e-9
    o = hr.opts(label_smoothing=0.1)
    assert hr.smooth_targets(o.label_smoothing) == (float(np.float32(cp)), float(np.float32(cn)))


# ---- the model ----

@pytest.mark.parametrize("name", list(hr.OPTION_SETS))
def test_the_closed_form_gradient_is_float64_autograd(name):
    """round_p=False: plain float64 throughout.  1e-8 of the kind-independent largest element: torch's BCELoss backward clamps with
    float32(1e-12) = 9.99999996e-13 in every dtype, the model (like loss_model64) with 1e-12; the two differ by 4e-9 relative where the
    clamp acts (set S), and by rounding elsewhere."""
    o = hr.OPTION_SETS[name]
    for c in _cases_of(name):
        m = hr.model(c, o, round_p=False)
        d = hr.head_loss(c, o, torch.float64)
        g, w = d["grad"].ravel(), m["grad"].ravel()
        assert np.isfinite(w).all() and np.abs(g - w).max() <= 1e-8 * max(np.abs(w).max(), 1e-300), (c.name, np.abs(g - w).max())
        for k in ("conf", "cls"):
            a, b = float(d[k]), float(m[k])
            assert (np.isnan(a) and np.isnan(b)) or abs(a - b) <= 1e-12 * max(abs(b), 1.0), (c.name, k, a, b)
        assert np.array_equal(d["tobj"], m["tobj"]), c.name
        r = hr.head_loss(c, o, torch.float64, round_p=True)          # and on rounded sigmoids, what `reference` uses for the defects
        w = hr.model(c, o)["grad"].ravel()
        assert np.abs(r["grad"].ravel() - w).max() <= 1e-8 * max(np.abs(w).max(), 1e-300), c.name


def test_neutral_options_are_the_existing_models_exactly():
    for c in JUDGED:
        for o in (hr.NEUTRAL, hr.opts(fl_alpha=0.9)):
            r = hr.reference(c, o)
            m = lc.reference(c)["m64"]
            assert np.array_equal(r["losses"], m["losses"], equal_nan=True) and np.array_equal(r["grad"].ravel(), m["grad"].ravel()), c.name
            for kind in br.KINDS:
                r, b = hr.reference(c, o._replace(box=kind)), br.reference(c, kind)
                assert np.array_equal(r["losses"], b["losses"], equal_nan=True) and np.array_equal(r["grad"].ravel(), b["grad"].ravel()), (c.name, kind)


def test_added_cases_have_the_property_they_name():
    for kind in br.KINDS:                                            # value < 0: the target clamps to 1 - g; value ~ 1: the target ~ 1
        for g in (1.0, 0.5):
            o = hr.opts(obj_iou=g, box=kind)
            c = hr.case_by_name("disjoint")
            pos = lc.reference(c)["planes"][0].numpy() == 1
            assert (br.reference(c, kind)["values"] < 0).all()
            assert (hr.reference(c, o)["tobj"][pos] == np.float32(1.0 - g)).all() and (hr.reference(c, o)["twin_tobj"][pos] == np.float32(1.0 - g)).all()
            c = hr.case_by_name("match")
            pos = lc.reference(c)["planes"][0].numpy() == 1
            t = hr.reference(c, o)["tobj"][pos]
            assert ((t >= 1 - 1e-5) & (t <= 1)).all()
    c = hr.case_by_name("pos_noobj")
    p = lc.reference(c)["planes"]
    both = (p[0].numpy() == 1) & (p[1].numpy() == 1)
    assert both.sum() >= 2 and ((p[0].numpy() == 1) & (p[1].numpy() == 0)).sum() >= 1
    c = hr.case_by_name("multi_hot")
    p = lc.reference(c)["planes"]
    hot = p[6].numpy()[p[0].numpy() == 1]
    assert sorted(hot.sum(1).tolist()) == [1.0, 2.0] and hot[hot.sum(1) == 2][0].tolist() == [1.0, 0.0, 1.0]
    c = hr.case_by_name("sat_pos")
    pos = lc.reference(c)["planes"][0].numpy() == 1
    x = c.logits.reshape(c.N, c.A, 5 + c.C, c.fh, c.fw).transpose(0, 1, 3, 4, 2)[pos][:, 4:]
    with np.errstate(over="ignore"):
        s = (1.0 / (1.0 + np.exp(-x.astype(np.float64)))).astype(np.float32)
    assert len(x) == 12 and np.isin(x, lc.S_VALUES).sum() == 36 and (s == 0).sum() >= 3 and (s == 1).sum() >= 6
    o = hr.OPTION_SETS["gamma1.5"]
    # there (1 - p_t) is exactly 0 or 1 at a 0 / 1 target
    t = np.stack([np.ones(len(x))] + list(lc.reference(c)["planes"][6].numpy()[pos].T), 1)
    q = 1.0 - (t * s + (1 - t) * (1 - s.astype(np.float64)))
    assert ((q == 0) | (q == 1))[(s == 0) | (s == 1)].all() and (q == 0).any() and (q == 1).any() and o.fl_gamma == 1.5


@pytest.mark.parametrize("name", list(hr.OPTION_SETS))
def test_every_judged_case_is_finite_and_the_twin_meets_its_condition(name):
    bad = []
    for c in _cases_of(name):
        ref = hr.reference(c, name)
        for what in ("losses", "twin_losses"):
            v = ref[what]
            assert np.isfinite(v[1:6]).all(), (c.name, what, v)
            assert bool(np.isfinite(v[[0, 6]]).all()) == (ref["n_pos"] > 0), (c.name, what, v)
        assert np.isfinite(ref["grad"]).all() and np.isfinite(ref["twin_grad"]).all(), c.name
        bad += hr.twin_condition(c, name)
    assert not bad, "\n".join(bad)


def test_what_the_widened_table_condition_lets_in(capsys):
    """twin_condition has two allowances loss_cases.twin_condition has not (one 2^-24 step of 1 - p_t under focal; the twin's own float32
    IoU values in t_obj).  Without them exactly these fail, all under `all` / `all_ref`, by the printed amounts -- cases the issue's table
    must keep: loss_cases' a8c20 and thres, each a few per cent of one floor over, and sat_pos."""
    found = {}
    for name in hr.OPTION_SETS:
        for c in _cases_of(name):
            for line in hr.twin_condition(c, name, widened=False):
                found.setdefault((name, c.name), []).append(line)
    with capsys.disabled():
        print("\n[loss options: outside the table condition without its two added allowances]\n" + "\n".join("  %-8s %s" % (k[0], v) for k, vs in found.items() for v in vs))
    assert set(found) == {("all", "a8c20"), ("all", "thres"), ("all", "sat_pos"), ("all_ref", "a8c20"), ("all_ref", "thres")}
    assert all(" grad " in v and " loss " not in v for vs in found.values() for v in vs)


def test_the_model_itself_passes_the_comparator():
    for name in hr.OPTION_SETS:
        for c in (hr.cases() if name.startswith("all") else SUBSET):
            r = hr.reference(c, name)
            l8 = np.array(list(r["losses"]) + [r["counted"]], np.float32)
            rep = hr.judge(c, name, l8, r["grad"].astype(np.float32))
            assert rep.ok, rep.failures


# which option set arms a defect, and a case that must be among those rejecting it
ARMED = {"mod_detached": ("all", None), "alpha_on_negatives": ("all", None), "pw_on_negatives": ("all", None),
         "smooth_negatives_zero": ("all", "multi_hot"), "iou_grad": ("all", None), "iou_unclamped": ("gr_giou", "disjoint"),
         "noobj_unmodulated": ("all", None), "gain_on_reported": ("all", None)}


def test_the_comparator_rejects_every_planted_defect(capsys):
    assert set(ARMED) == set(hr.DEFECTS)
    lines = []
    for defect in hr.DEFECTS:
        name, must = ARMED[defect]
        rejected = []
        for c in SUBSET:
            d = hr.reference(c, name, defect=defect)
            l8 = np.array(list(d["losses"]) + [d["counted"]], np.float32)
            if not hr.judge(c, name, l8, d["grad"].astype(np.float32)).ok:
                rejected.append(c.name)
        lines.append("  %-22s %-8s rejected on %d of %d cases: %s" % (defect, name, len(rejected), len(SUBSET), ", ".join(rejected[:8])))
        assert rejected and (must is None or must in rejected), (defect, rejected)
    with capsys.disabled():
        print("\n[loss options: planted defects]\n" + "\n".join(lines))


# ---- the term header on the host ----

def _compiler():
    for name in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/bin/amdclang++"):
        path = shutil.which(name)
        if path:
            return path
    raise AssertionError("no C++ compiler found (the build needs one)")


def test_the_kernels_loss_term_on_the_host_against_float64_autograd(tmp_path, capsys):
    """element to 1e-12 of max(|element|, 1); derivative to 1e-8 relative (torch's float32(1e-12) clamp constant, see above) plus 1e-12"""
    csrc = os.path.join(ROOT, "yolo-fastest-and-embedded-deployment_amd", "csrc")
    exe = str(tmp_path / "loss_term_host")
    subprocess.check_call([_compiler(), "-O2", "-ffp-contract=off", "-I", csrc, "-o", exe, os.path.join(ROOT, "tests", "loss_term_host.cpp")])
    f32 = np.float32
    with np.errstate(over="ignore"):
        ps = [0.0, 1.0, float(np.nextafter(f32(1), f32(0))), float(np.nextafter(f32(0), f32(1))), 1e-30, 2e-9, 0.5] + \
            [float(f32(1 / (1 + np.exp(-v)))) for v in np.linspace(-12, 12, 25)]
    ts = [0.0, 1.0, float(f32(0.95)), float(f32(0.05)), 0.3, float(np.nextafter(f32(1), f32(0)))]
    recs = [(p, t, w, gamma, alpha) for p in ps for t in ts for w in (1.0, 0.6, 2.5) for gamma, alpha in ((0.0, 0.25), (1.0, 0.25), (1.5, 0.3), (2.0, 0.7), (5.0, 1.0))]
    np.array(recs, np.float64).tofile(str(tmp_path / "in.bin"))
    subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    out = np.fromfile(str(tmp_path / "out.bin"), np.float64).reshape(-1, 2)
    assert len(out) == len(recs) > 2000 and np.isfinite(out).all()
    worst = [0.0, 0.0]
    for (gamma, alpha, w) in sorted({(r[3], r[4], r[2]) for r in recs}):
        idx = [i for i, r in enumerate(recs) if (r[3], r[4], r[2]) == (gamma, alpha, w)]
        p = torch.tensor([recs[i][0] for i in idx], dtype=torch.float64, requires_grad=True)
        t = torch.tensor([recs[i][1] for i in idx], dtype=torch.float64)
        e = hr.element(p, t, w, hr.opts(fl_gamma=gamma, fl_alpha=alpha))
        e.sum().backward()
        de = np.abs(out[idx, 0] - e.detach().numpy()) / np.maximum(np.abs(e.detach().numpy()), 1.0)
        dd = np.abs(out[idx, 1] - p.grad.numpy()) / (1e-8 * np.abs(p.grad.numpy()) + 1e-12)
        worst = [max(worst[0], de.max()), max(worst[1], dd.max())]
        assert de.max() <= 1e-12 and dd.max() <= 1.0, (gamma, alpha, w, de.max(), dd.max())
    with capsys.disabled():
        print("\n[loss term on the host: %d records; element off by at most %.1e, derivative at most %.2f of its allowance]" % (len(recs), *worst))


# ---- the surface ----

def test_the_abi_names_the_hyp_entries():
    hdr = open(os.path.join(ROOT, "include", "yolo_fastest_hip.h")).read()
    for text in ("int yf_train_head_loss_hyp_workspace_bytes(", "int yf_train_head_loss_hyp(", "double obj_pw, double cls_pw,",
                 "double label_smoothing, double fl_gamma, double fl_alpha, double obj_iou, double lambda_conf, double lambda_cls);"):
        assert text in hdr, text
    from yolo_fastest_amd import _lib, validation
    assert "yf_train_head_loss_hyp" in _lib.EXPORTS and "yf_train_head_loss_hyp_workspace_bytes" in _lib.EXPORTS
    assert len(_lib._SIGS["yf_train_head_loss_hyp"][1]) == len(_lib._SIGS["yf_train_head_loss_box"][1]) + 8
    assert _lib._SIGS["yf_train_head_loss_hyp_workspace_bytes"] == _lib._SIGS["yf_train_head_loss_box_workspace_bytes"]
    assert tuple(n for n, _ in validation.LOSS_HYP_DEFAULTS) == hr.OPTION_NAMES
    assert tuple(v for _, v in validation.LOSS_HYP_DEFAULTS) == tuple(hr.NEUTRAL[:8])


def _crit(**kw):
    from yolo_fastest_amd import validation
    return validation.YOLOLossV3(lc.ANC_LARGE, 3, [64, 96, 1], "cpu", **kw)


REFUSED = [dict(obj_pw=0.0), dict(obj_pw=-1.0), dict(cls_pw=0.0), dict(label_smoothing=-0.1), dict(label_smoothing=1.5), dict(fl_gamma=-1.0),
           dict(fl_gamma=0.5), dict(fl_gamma=0.999), dict(fl_alpha=-0.1), dict(fl_alpha=1.1), dict(obj_iou=-0.1, box_loss="ciou"),
           dict(obj_iou=1.1, box_loss="ciou"), dict(obj_iou=0.5), dict(lambda_conf=-1.0), dict(lambda_cls=-1e-9)] + \
          [{k: v} for k in hr.OPTION_NAMES for v in (float("nan"), float("inf"))]


@pytest.mark.parametrize("kw", REFUSED, ids=lambda kw: ",".join("%s=%r" % i for i in kw.items()))
def test_YOLOLossV3_refuses_what_the_entry_refuses(kw):
    with pytest.raises(ValueError):
        _crit(**kw)


def test_YOLOLossV3_defaults_and_accepted_values():
    crit = _crit()
    assert crit.loss_hyp == tuple(hr.NEUTRAL[:8]) and crit.box_loss is None
    o = hr.OPTION_SETS["all"]
    crit = _crit(box_loss="ciou", **dict(zip(hr.OPTION_NAMES, o[:8])))
    assert crit.loss_hyp == tuple(o[:8])
    _crit(fl_gamma=1.0, label_smoothing=1.0, lambda_conf=0.0, lambda_cls=0.0, fl_alpha=0.0)


def test_train_refuses_bad_loss_hyp(tmp_path):
    import yolo_fastest_amd as yf
    from yolo_fastest_amd import training
    params = copy.deepcopy(yf.config_params)
    params["io_params"]["save_path"] = str(tmp_path / "models")
    items = [object()]                                             # never read
    assert set(training.LOSS_HYP_KEYS) == {"obj", "cls", "obj_pw", "cls_pw", "fl_gamma", "label_smoothing", "gr", "fl_alpha"}
    with pytest.raises(ValueError, match="anchor_t"):
        training.train(params, None, train_dataset=items, loss_hyp={"obj": 1.0, "anchor_t": 4.0})
    with pytest.raises(ValueError, match="box_loss"):
        training.train(params, None, train_dataset=items, loss_hyp={"gr": 1.0})
    for bad in ({"fl_gamma": 0.5}, {"obj": -1.0}, {"cls_pw": 0.0}, {"label_smoothing": 2.0}, {"gr": 1.5}, {"fl_alpha": float("nan")}):
        with pytest.raises(ValueError):
            training.train(params, None, train_dataset=items, box_loss="ciou", loss_hyp=bad)
    assert not os.path.exists(params["io_params"]["save_path"])    # refused before anything is built
    assert "PLAIN gains" in training.train.__doc__                 # obj / cls are not yolov5's rescaled ones, and the docstring says so
