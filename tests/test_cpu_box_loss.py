"""The definition side of the IoU-family box loss (tests/box_loss_ref.py; the kernels are held to it in tests/test_gpu_box_loss.py),
without a GPU:

  * the four hand checks of the definition, to 1e-6;
  * every judged case of the table (loss_cases.cases() plus box_loss_ref.added_cases()) is finite for all three kinds, model and twin
    (cls and total NaN without a positive cell, as documented), and every added case has the property it names;
  * `clamp`: the w / h gradient is exactly zero outside [-10, 10] and non-zero at +-10 and inside;
  * no judged case has a positive cell where two arguments of a min / max, or an extent and 0, are equal in float64 (autograd's
    subgradient at a tie is a convention; `match`, which ties by construction, is judged on losses and finiteness only);
  * csrc/yf_box_term.h -- the function the kernel calls per positive cell, compiled for the host -- gives the model's value to 1e-12 and
    its hand-derived gradient to 1 % of the float32 floor the device is held to (both are float64 evaluations of one derivative; what
    separates them must vanish against the half ulp the float32 store alone costs, which is 12.5 % of that floor);
  * the comparator rejects five planted defects: alpha differentiated, normalised by n_pos, the clamp's gradient passed through, gw
    taken from the first target of a cell, corners built from w instead of w / 2;
  * the twin's distance per case is printed (test_twin_distance).  MEASURED: on loss_cases' table the twin's `box` gradient is at
    most 3.9 of the 4-ulp floors away from the model, with one outlier: giou / e3_S, 68,000 floors (4.3e-8 on a gradient whose largest
    element is 1.9e-6) -- float32 cancels in GIoU's enclosing-area term for a clamped, huge box, which is why the kernel evaluates the
    term in double.  Of the added cases `clamp` (huge boxes on purpose) shows the same under giou, 3,700 floors, and `disjoint` 9.1;
    the host build of the kernel's function is 2.5e-4 of a floor away on its worst cell.
"""
import math
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

JUDGED = br.judged_cases()
ADDED = {c.name: c for c in br.added_cases()}

HAND = [((0, 0, 2, 2), (1, 0, 2, 2), (0.3333333, 0.2564103, 0.2564103)),
        ((0, 0, 4, 1), (0, 0, 1, 4), (-0.4196429, 0.1428571, -0.0256105)),
        ((0, 0, 1, 1), (3, 4, 1, 2), (-0.8636364, -0.5405405, -0.5422300)),
        ((0.5, 0.5, 1, 1), (0.6, 0.4, 4, 2), (0.1250000, 0.1240000, 0.1220802))]


@pytest.mark.parametrize("b1,b2,want", HAND)
def test_hand_checks(b1, b2, want):
    args = [torch.tensor([float(v)], dtype=torch.float64) for v in b1 + b2]
    for kind, w in zip(br.KINDS, want):
        assert abs(float(br.iou_family(*args, kind)) - w) <= 1e-6, (kind, b1, b2)


def _cells(c):
    """per positive cell, float64: logits [P, 4], anchors [P, 2], (tx, ty, gw, gh) [P, 4]"""
    ref = lc.reference(c)
    (n, a, j, k), gw, gh = br.positives(c, ref)
    x = c.logits.reshape(c.N, c.A, 5 + c.C, c.fh, c.fw).astype(np.float64)
    t = x[n, a, :, j, k][:, :4].reshape(-1, 4)
    anc = lc.anchors32(c).astype(np.float64)[a]
    tgt = np.stack([ref["planes"][2].numpy()[n, a, j, k], ref["planes"][3].numpy()[n, a, j, k], gw[n, a, j, k], gh[n, a, j, k]], 1).astype(np.float64)
    return t, anc, tgt.reshape(-1, 4), (n, a, j, k)


@pytest.mark.parametrize("kind", br.KINDS)
def test_every_judged_case_is_finite(kind):
    for c in JUDGED:
        ref = br.reference(c, kind)
        for what in ("losses", "twin_losses"):
            v = ref[what]
            assert np.isfinite(v[1:6]).all(), (c.name, what, v)
            assert bool(np.isfinite(v[[0, 6]]).all()) == (ref["n_pos"] > 0), (c.name, what, v)
        assert np.isfinite(ref["grad"]).all() and np.isfinite(ref["twin_grad"]).all() and np.isfinite(ref["values"]).all(), c.name
        if ref["n_pos"] == 0:
            assert ref["losses"][1] == 0.0 and ref["twin_losses"][1] == 0.0


def test_added_cases_have_the_property_they_name():
    def geometry(name):
        t, anc, g, _ = _cells(ADDED[name])
        px, py = 1 / (1 + np.exp(-t[:, 0])), 1 / (1 + np.exp(-t[:, 1]))
        pw, ph = np.exp(np.clip(t[:, 2], -10, 10)) * anc[:, 0], np.exp(np.clip(t[:, 3], -10, 10)) * anc[:, 1]
        return (px - pw / 2, px + pw / 2, py - ph / 2, py + ph / 2), (g[:, 0] - g[:, 2] / 2, g[:, 0] + g[:, 2] / 2, g[:, 1] - g[:, 3] / 2, g[:, 1] + g[:, 3] / 2)
    a, b = geometry("disjoint")
    assert len(a[0]) == 2 and ((a[1] < b[0]) & (a[3] < b[2])).all()                       # apart in x and in y
    assert (b[0] > 0).all() and (b[1] < 1).all() and (a[0] > 0).all() and (a[3] < 1).all()   # both inside the one cell
    a, b = geometry("pred_inside")
    assert ((a[0] > b[0]) & (a[1] < b[1]) & (a[2] > b[2]) & (a[3] < b[3])).all()
    a, b = geometry("target_inside")
    assert ((a[0] < b[0]) & (a[1] > b[1]) & (a[2] < b[2]) & (a[3] > b[3])).all()
    a, b = geometry("aspect")
    assert (a[0] + a[1] == b[0] + b[1]).all() and (a[2] + a[3] == b[2] + b[3]).all()      # equal centres, exactly
    assert ((a[1] - a[0] < b[1] - b[0]) & (a[3] - a[2] > b[3] - b[2])).all()              # crossed shapes
    assert abs(br.reference(ADDED["aspect"], "ciou")["values"][0] - br.reference(ADDED["aspect"], "diou")["values"][0]) > 1e-2
    t, _, _, _ = _cells(ADDED["clamp"])
    assert sorted(set(np.float32(t[:, 2:4]).ravel().tolist())) == sorted(float(v) for v in br._clamp_values())
    c = ADDED["last_wins"]
    _, _, g, _ = _cells(c)
    assert g.shape[0] == 1 and g[0, 2] == float(c.targets[0, 1, 2] * np.float32(6)) != float(c.targets[0, 0, 2] * np.float32(6))
    for kind in br.KINDS:
        assert (br.reference(ADDED["match"], kind)["values"] >= 1 - 1e-5).all()
        assert (br.reference(ADDED["disjoint"], kind)["values"] < 0).all()


@pytest.mark.parametrize("kind", br.KINDS)
def test_clamp_gradient_is_zero_outside_and_not_at_the_ends(kind):
    c = ADDED["clamp"]
    t, _, _, (n, a, j, k) = _cells(c)
    seen = set()
    for what in ("grad", "twin_grad"):
        g = br.reference(c, kind)[what].reshape(c.N, c.A, 5 + c.C, c.fh, c.fw)[n, a, :, j, k][:, 2:4]
        for v, d in zip(t[:, 2:4].ravel(), g.ravel()):
            if what == "grad" or abs(v) > 10.0:             # (in float32 a huge box's GIoU gradient may cancel to 0 inside the clamp too)
                assert (d == 0.0) == (abs(v) > 10.0), (what, v, d)
            seen.add(float(v))
    assert {10.0, -10.0} <= seen and any(abs(v) > 10 for v in seen)


def test_no_judged_case_sits_on_a_tie():
    for c in JUDGED:
        if c.name in br.LOSSES_ONLY:
            continue
        t, anc, g, _ = _cells(c)
        if not len(t):
            continue
        with np.errstate(over="ignore"):
            px, py = 1 / (1 + np.exp(-t[:, 0])), 1 / (1 + np.exp(-t[:, 1]))
        pw, ph = np.exp(np.clip(t[:, 2], -10, 10)) * anc[:, 0], np.exp(np.clip(t[:, 3], -10, 10)) * anc[:, 1]
        for lo1, hi1, lo2, hi2 in ((px - pw / 2, px + pw / 2, g[:, 0] - g[:, 2] / 2, g[:, 0] + g[:, 2] / 2),
                                   (py - ph / 2, py + ph / 2, g[:, 1] - g[:, 3] / 2, g[:, 1] + g[:, 3] / 2)):
            assert not (lo1 == lo2).any() and not (hi1 == hi2).any(), c.name
            assert not (np.minimum(hi1, hi2) - np.maximum(lo1, lo2) == 0).any(), c.name


def _compiler():
    for name in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/bin/amdclang++"):
        path = shutil.which(name)
        if path:
            return path
    raise AssertionError("no C++ compiler found (the build needs one)")


def test_the_kernels_box_term_on_the_host_against_float64_autograd(tmp_path, capsys):
    csrc = os.path.join(ROOT, "yolo-fastest-and-embedded-deployment_amd", "csrc")
    exe = str(tmp_path / "box_term_host")
    subprocess.check_call([_compiler(), "-O2", "-ffp-contract=off", "-I", csrc, "-o", exe, os.path.join(ROOT, "tests", "box_term_host.cpp")])
    recs, want = [], []
    for c in JUDGED:
        if c.name in br.LOSSES_ONLY:
            continue
        t, anc, g, (n, a, j, k) = _cells(c)
        E = c.N * c.A * c.fh * c.fw
        for kind in br.KINDS:
            ref = br.reference(c, kind)
            grad = ref["grad"].reshape(c.N, c.A, 5 + c.C, c.fh, c.fw)[n, a, :, j, k][:, :4].reshape(-1, 4)
            for i in range(len(t)):
                recs.append([br.KIND_ID[kind], *t[i], *anc[i], *g[i]])
                want.append((c.name, kind, ref["values"][i], grad[i], -br.LAMBDA_BOX / E))
    np.array(recs, np.float64).tofile(str(tmp_path / "in.bin"))
    subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    out = np.fromfile(str(tmp_path / "out.bin"), np.float64).reshape(-1, 5)
    assert len(out) == len(want) > 1000
    err, top = {}, {}
    for (name, kind, v, g, scale), o in zip(want, out):
        assert abs(o[0] - v) <= 1e-12, (name, kind, o[0], v)
        key = (name, kind)
        err[key] = max(err.get(key, 0.0), float(np.abs(scale * o[1:] - g).max()))
        top[key] = max(top.get(key, 0.0), float(np.abs(g).max()))
    ratio = {k: err[k] / (lc.GRAD_ULPS * lc.ulp32(top[k])) for k in err if top[k] > 0}
    worst = max(ratio, key=ratio.get)
    with capsys.disabled():
        print("\n[box term on the host: %d cells; worst gradient distance %.2e of the 4-ulp floor (%s %s)]" % (len(out), ratio[worst], *worst))
    assert ratio[worst] <= 0.01


def test_the_comparator_rejects_every_planted_defect(capsys):
    lines = []
    for defect in br.DEFECTS:
        for kind in br.KINDS:
            if defect == "alpha_grad" and kind != "ciou":
                continue
            rejected = []
            for c in JUDGED:
                d = br.reference(c, kind, defect=defect)
                l8 = np.array(list(d["losses"]) + [d["counted"]], np.float32)
                if not br.judge(c, kind, l8, d["grad"].astype(np.float32)).ok:
                    rejected.append(c.name)
            lines.append("  %-18s %-5s rejected on %d cases: %s" % (defect, kind, len(rejected), ", ".join(rejected[:6])))
            assert rejected, (defect, kind)
            if defect == "clamp_passthrough":
                assert "clamp" in rejected
            if defect == "gw_first":
                assert "last_wins" in rejected
    with capsys.disabled():
        print("\n[box loss: planted defects]\n" + "\n".join(lines))


def test_the_model_itself_passes_the_comparator():
    for kind in br.KINDS:
        for c in br.cases():
            r = br.reference(c, kind)
            l8 = np.array(list(r["losses"]) + [r["counted"]], np.float32)
            rep = br.judge(c, kind, l8, r["grad"].astype(np.float32))
            assert rep.ok, rep.failures


def test_twin_distance(capsys):
    """prints, per kind, the twin's distance to the model in units of the floors (8 ulps of the loss, 4 ulps of the gradient kind's maximum)"""
    lines, worst = [], {}
    for kind in br.KINDS:
        for c in JUDGED:
            r = br.reference(c, kind)
            if r["n_pos"] == 0:
                continue
            sel = r["kinds"]["box"].reshape(r["grad"].shape)
            top = np.abs(r["grad"][sel]).max()
            gd = np.abs(r["twin_grad"][sel] - r["grad"][sel]).max() / (lc.GRAD_ULPS * lc.ulp32(top))
            ld = abs(float(r["twin_losses"][1]) - r["losses"][1]) / (lc.LOSS_ULPS * lc.ulp32(r["losses"][1]))
            lines.append("  %-5s %-14s loss box %.2f floors, grad box %.2f floors (largest element %.2e)" % (kind, c.name, ld, gd, top))
            worst[(kind, c.name)] = gd
    with capsys.disabled():
        print("\n[box loss: the float32 twin against the float64 model]\n" + "\n".join(lines))
    assert all(math.isfinite(v) for v in worst.values())


def test_the_abi_names_the_box_entries():
    """header, export table and constants agree (no library needed)"""
    hdr = open(os.path.join(ROOT, "include", "yolo_fastest_hip.h")).read()
    for text in ("#define YF_BOX_REF 0", "#define YF_BOX_GIOU 1", "#define YF_BOX_DIOU 2", "#define YF_BOX_CIOU 3", "#define YF_BOX_WH_CLAMP 10.0",
                 "#define YF_ABI_VERSION 1", "int yf_train_head_loss_box_workspace_bytes(", "int yf_train_head_loss_box("):
        assert text in hdr, text
    from yolo_fastest_amd import _lib, validation
    assert "yf_train_head_loss_box" in _lib.EXPORTS and "yf_train_head_loss_box_workspace_bytes" in _lib.EXPORTS
    assert len(_lib._SIGS["yf_train_head_loss_box"][1]) == len(_lib._SIGS["yf_train_head_loss_ex"][1]) + 2
    assert validation.BOX_KINDS == br.KIND_ID
    with pytest.raises(ValueError):
        validation.YOLOLossV3(lc.ANC_LARGE, 3, [64, 96, 1], "cpu", box_loss="siou")
    with pytest.raises(ValueError):
        validation.YOLOLossV3(lc.ANC_LARGE, 3, [64, 96, 1], "cpu", box_loss="ciou", lambda_box=float("nan"))
    crit = validation.YOLOLossV3(lc.ANC_LARGE, 3, [64, 96, 1], "cpu")
    assert crit.box_loss is None and crit.lambda_box == 5.0
