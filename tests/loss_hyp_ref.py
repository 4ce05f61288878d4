"""yolov5's objectness / class loss options on one head (`yf_train_head_loss_hyp`: loss_cells_kernel<GRAD, BOX, true>, loss_final_kernel
in csrc/yf_loss_kernels.hip, csrc/yf_loss_term.h), stated once as a dtype-generic torch function, with its option sets, its case table
and its comparator.  Shared by tests/test_cpu_loss_hyp.py (the definition alone) and tests/test_gpu_loss_hyp.py (the kernels).

THE DEFINITION (`element`, `head_loss`; include/yolo_fastest_hip.h states it above the entry).  get_target, the masks, the box terms and
the normalisations are untouched; only the BCE element and its targets change.  p = a sigmoid times its mask, t the target, w the weight:
  base      -(w t max(log p, -100) + (1 - t) max(log(1 - p), -100)), written as w t BCE(p, 1) + (1 - t) BCE(p, 0) with torch's BCELoss, whose
            backward carries torch's clamp: d base / d p = (-w t (1 - p) + (1 - t) p) / max((1 - p) p, 1e-12)
  focal     gamma > 0 only: elem = base * (t alpha + (1 - t)(1 - alpha)) * (1 - p_t)^gamma, p_t = t p + (1 - t)(1 - p), the modulating
            factor differentiated; on every element of conf_obj, conf_noobj and cls
  weights   obj_pw on conf_obj, cls_pw on cls (conf_noobj has target 0)
  smoothing class targets float32(1 - eps / 2) where the plane is 1, float32(eps / 2) where it is 0
  t_obj     at a positive cell float32((1 - g) + g clamp(value, 0, 1)), value the cell's GIoU / DIoU / CIoU, detached; needs a box kind
  total     [2.5 (x + y + w + h) or lambda_box box] + lambda_conf conf + lambda_cls cls; the reported conf and cls stay unweighted

MODEL (`reference(case, name)["losses" / "grad"]`): the definition in float64 on float32-ROUNDED sigmoids (oracle.loss_oracle.loss_model64's
"float64 that rounds where fp32 must"), with a closed-form numpy gradient (`_elem_np`, `_core`); test_cpu_loss_hyp.py pins every formula
to float64 autograd of `head_loss`.  The box channels, the box losses and the IoU values come from box_loss_ref (loss_cases for YF_BOX_REF).
TWIN: `head_loss` in float32 with torch autograd, its own float32 sigmoids and its own float32 IoU values.

OPTION SETS (`OPTION_SETS`): each knob alone (fl_alpha alone is not read, so it rides on gamma = 2), gamma of 1, 1.5 and 2, and `all`: every
knob away from neutral with g = 1 under CIoU, plus `all_ref`: the same under YF_BOX_REF with g = 0 (g > 0 is refused there).

CASES: box_loss_ref.cases() (loss_cases' table plus its own seven, among them `disjoint`: every IoU value below 0, so t_obj clamps to
1 - g, and `match`: t_obj within 1e-5 of 1) plus, on a 4x6 map with N <= 2 (`added_cases`):
  pos_noobj   a target so large that no anchor's IoU exceeds the ignore threshold: the positive cell keeps noobj_mask = 1 and both
              confidence elements act on one logit
  multi_hot   two targets of different classes in one cell with one best anchor: a two-hot class plane under smoothing
  sat_pos     confidence and class logits of set S at the positive cells: p exactly 0 or 1, where (1 - p_t) is exactly 0 or 1 under focal
              (one class logit per cell stays of set M, so that the kind's largest gradient is not itself a rounding residue)

THE COMPARATOR (`judge`), loss_cases.py's numbers unchanged:
  losses   |dev - m64| <= max(3 |twin - m64|, 8 float32 ulps of |m64|); NaN exactly where the model has NaN; [7] exact; with a box kind
           d_losses[2..4] exactly 0
  grad     per kind: max|dev - m64| <= max(3 max|twin - m64|, 4 float32 ulps of the kind's max|m64|); box_off, conf_ignored, cls_off exactly
           zero.  (Only those three: under YF_BOX_REF box_loss_ref's `match` has a model gradient of exactly 0 in the kinds x and y too,
           because float32(sigmoid(logit(tx))) happens to be tx at each of its cells; a sigmoid one float32 step off is not a defect,
           and the first rule holds it.)  Under a box kind box_loss_ref's `match` (its corners tie, where the box subgradient is a convention) is not judged on the
           kind `box`; its other kinds are.
No bound comes from what the device computes.  `twin_condition` is what the table itself must satisfy for conf, cls and their gradient
kinds: the twin within the ulp floors alone plus what the number format is worth to the model (its docstring lists the three allowances).
"""
import collections
import math

import numpy as np
import torch
import torch.nn.functional as F

import box_loss_ref as br
import loss_cases as lc
from oracle import loss_oracle as lo

F32 = np.float32
Opts = collections.namedtuple("Opts", "obj_pw cls_pw label_smoothing fl_gamma fl_alpha obj_iou lambda_conf lambda_cls box lambda_box")
NEUTRAL = Opts(1.0, 1.0, 0.0, 0.0, 0.25, 0.0, 1.0, 1.0, None, br.LAMBDA_BOX)
OPTION_NAMES = Opts._fields[:8]                               # the entry's argument order


def opts(**kw):
    return NEUTRAL._replace(**kw)


OPTION_SETS = collections.OrderedDict([
    ("obj_pw", opts(obj_pw=2.5)),
    ("cls_pw", opts(cls_pw=0.6)),
    ("smooth", opts(label_smoothing=0.1)),
    ("gamma1", opts(fl_gamma=1.0)),
    ("gamma1.5", opts(fl_gamma=1.5)),
    ("gamma2", opts(fl_gamma=2.0)),
    ("alpha", opts(fl_gamma=2.0, fl_alpha=0.7)),
    ("gr_giou", opts(obj_iou=1.0, box="giou")),
    ("gr_half", opts(obj_iou=0.5, box="diou")),
    ("lambda_conf", opts(lambda_conf=0.7)),
    ("lambda_cls", opts(lambda_cls=1.3, box="ciou")),
    ("all", Opts(1.7, 0.6, 0.1, 1.5, 0.3, 1.0, 0.7, 1.3, "ciou", br.LAMBDA_BOX)),
    ("all_ref", Opts(1.7, 0.6, 0.1, 1.5, 0.3, 0.0, 0.7, 1.3, None, br.LAMBDA_BOX)),
])
SINGLE_KNOB = tuple(k for k in OPTION_SETS if not k.startswith("all"))
DEFECTS = ("mod_detached", "alpha_on_negatives", "pw_on_negatives", "smooth_negatives_zero", "iou_grad", "iou_unclamped", "noobj_unmodulated",
           "gain_on_reported")
BOX_TIES = br.LOSSES_ONLY
ALWAYS_ZERO = ("box_off", "conf_ignored", "cls_off")          # the kinds whose gradient is zero in exact arithmetic: held to an exact 0


def smooth_targets(eps):
    """(cp, cn) as the entry forms them: in double, rounded to float32 once"""
    return float(F32(1.0 - 0.5 * eps)), float(F32(0.5 * eps))


# ---- the definition ----

def element(p, t, w, o, defect=None, modulate=True):
    """one BCE element under the options; tensors of one dtype, p in [0, 1]"""
    pos = F.binary_cross_entropy(p, torch.ones_like(p), reduction="none")         # -max(log p, -100); backward (p - 1) / max((1 - p) p, 1e-12)
    neg = F.binary_cross_entropy(p, torch.zeros_like(p), reduction="none")        # -max(log(1 - p), -100)
    base = (t * pos + w * (1 - t) * neg) if defect == "pw_on_negatives" else (w * t * pos + (1 - t) * neg)
    if o.fl_gamma > 0 and modulate:
        p_t = t * p + (1 - t) * (1 - p)
        af = (t * (1 - o.fl_alpha) + (1 - t) * o.fl_alpha) if defect == "alpha_on_negatives" else (t * o.fl_alpha + (1 - t) * (1 - o.fl_alpha))
        mod = (1 - p_t) ** o.fl_gamma
        base = base * af * (mod.detach() if defect == "mod_detached" else mod)
    return base


class _RoundedSigmoid(torch.autograd.Function):
    """float64 in, float32(sigmoid) widened out; backward (1 - p) p of the ROUNDED p, as a kernel that only ever sees the float32 has it"""

    @staticmethod
    def forward(ctx, x):
        p = torch.sigmoid(x).float().double()
        ctx.save_for_backward(p)
        return p

    @staticmethod
    def backward(ctx, g):
        (p,) = ctx.saved_tensors
        return g * (1 - p) * p


def _positive_index(case):
    idx, gw, gh = br.positives(case)
    return tuple(torch.from_numpy(i) for i in idx), gw, gh


def head_loss(case, o, dtype, defect=None, round_p=False, logits=None):
    """The objectness and class part of one head under `o`, from the logits, in `dtype` -> dict: conf, cls (0-dim tensors, unweighted),
    grad (d(lambda_conf conf + lambda_cls cls) / d logits, float64 numpy like the logits), tobj (the objectness target plane, float64
    numpy).  round_p (float64 only): the sigmoids of channels 4.. are rounded to float32."""
    ref = lc.reference(case)
    m, nm = ref["planes"][0].to(dtype), ref["planes"][1].to(dtype)
    tc = ref["planes"][6].to(dtype)                                               # [N, A, h, w, C]
    x = torch.from_numpy(case.logits if logits is None else logits).to(dtype).requires_grad_(True)
    p5 = x.view(case.N, case.A, 5 + case.C, case.fh, case.fw)
    sig = _RoundedSigmoid.apply if round_p else torch.sigmoid
    pc, pk = sig(p5[:, :, 4]), sig(p5[:, :, 5:]).permute(0, 1, 3, 4, 2)
    tobj = m
    if o.obj_iou > 0:
        (n, a, j, k), gw, gh = _positive_index(case)
        t4 = p5[n, a, :, j, k][:, 0:4]
        anc = torch.from_numpy(lc.anchors32(case)).to(dtype)[a]
        tgt = torch.stack([ref["planes"][2][n, a, j, k], ref["planes"][3][n, a, j, k], torch.from_numpy(gw)[n, a, j, k],
                           torch.from_numpy(gh)[n, a, j, k]], 1).to(dtype)
        v = br.box_values(t4, anc, tgt, o.box)
        if defect != "iou_grad":
            v = v.detach()
        if defect != "iou_unclamped":
            v = v.clamp(0, 1)
        tpos = (1 - o.obj_iou) + o.obj_iou * v
        if dtype == torch.float64:
            tpos = tpos + (tpos.float().double() - tpos).detach()                 # the float32 the kernel forms
        tobj = torch.zeros_like(m).index_put((n, a, j, k), tpos)
    E = m.numel()
    conf_obj = element(pc * m, tobj, o.obj_pw, o, defect).sum() / E
    conf_noobj = element(pc * nm, nm * 0.0, 1.0, o, defect, modulate=defect != "noobj_unmodulated").sum() / E
    conf = conf_obj + 0.5 * conf_noobj
    cp, cn = smooth_targets(o.label_smoothing)
    if defect == "smooth_negatives_zero":
        cn = 0.0
    pos = m == 1
    tk = torch.where(tc == 1, torch.full_like(tc, cp), torch.full_like(tc, cn))
    cls = element(pk[pos], tk[pos], o.cls_pw, o, defect).mean()                   # NaN without a positive cell, like the reference's
    (o.lambda_conf * conf + o.lambda_cls * cls).backward()
    return dict(conf=conf.detach(), cls=cls.detach(), grad=x.grad.double().numpy(), tobj=tobj.detach().double().numpy())


# ---- the float64 model in closed form ----

def _elem_np(p, t, w, gamma, alpha, dq=0.0):
    """-> (element, d element / d p), float64 arrays.  dq: added to 1 - p_t (twin_condition's float32 step of it), kept >= 0"""
    base = -(w * t * np.maximum(np.log(p), -100.0) + (1.0 - t) * np.maximum(np.log(1.0 - p), -100.0))
    dbase = (-w * t * (1.0 - p) + (1.0 - t) * p) / np.maximum((1.0 - p) * p, 1e-12)
    if not gamma > 0:
        return base, dbase
    q = 1.0 - (t * p + (1.0 - t) * (1.0 - p))
    if dq:
        q = np.maximum(q + dq, 0.0)
    af = t * alpha + (1.0 - t) * (1.0 - alpha)
    mod, dmod = q ** gamma, gamma * q ** (gamma - 1.0) * (1.0 - 2.0 * t)
    return base * af * mod, af * (dbase * mod + base * dmod)


def _core(sig, case, ref, o, tobj, dq=0.0, parts=None):
    """sig float64 [N, A, 5 + C, h, w] (rounded or not), tobj float64 [N, A, h, w] (0 off the positive cells) -> (conf, cls, gradient of
    lambda_conf conf + lambda_cls cls like sig with channels 0..3 zero).  parts: a dict that receives the per-element terms, each already
    divided by its normalisation (conf [N, A, h, w], cls [N, A, C, h, w])"""
    m, nm = (ref["planes"][i].numpy().astype(np.float64) for i in (0, 1))
    tc = ref["planes"][6].numpy().astype(np.float64).transpose(0, 1, 4, 2, 3)
    C, E, n_pos, pos = case.C, float(m.size), float(m.sum()), m == 1
    pc, pk = sig[:, :, 4], sig[:, :, 5:]
    cp, cn = smooth_targets(o.label_smoothing)
    with np.errstate(divide="ignore", invalid="ignore"):
        e_obj, d_obj = _elem_np(pc * m, tobj, o.obj_pw, o.fl_gamma, o.fl_alpha, dq)
        e_no, d_no = _elem_np(pc * nm, nm * 0.0, 1.0, o.fl_gamma, o.fl_alpha, dq)
        e_cls, d_cls = _elem_np(pk, np.where(tc == 1, cp, cn), o.cls_pw, o.fl_gamma, o.fl_alpha, dq)
        if parts is not None:
            parts["conf"] = (e_obj + 0.5 * e_no) / E
            parts["cls"] = e_cls * pos[:, :, None] / (C * max(n_pos, 1.0))
        conf = e_obj.sum() / E + 0.5 * (e_no.sum() / E)
        cls = (e_cls * pos[:, :, None]).sum() / (C * n_pos) if n_pos else float("nan")
        g = np.zeros(sig.shape, np.float64)
        g[:, :, 4] = o.lambda_conf * ((d_obj * m + 0.5 * d_no * nm) * (1.0 - pc) * pc / E)
        if n_pos:
            g[:, :, 5:] = o.lambda_cls * (d_cls * (1.0 - pk) * pk / (C * n_pos) * pos[:, :, None])
    return conf, cls, g


def _sig64(case, logits=None):
    v = np.asarray(case.logits if logits is None else logits).reshape(case.N, case.A, 5 + case.C, case.fh, case.fw).astype(np.float64)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-v))


def _tobj(case, ref, o, values):
    """the objectness target plane, float64: 1 at the positive cells, or float32((1 - g) + g clamp(value, 0, 1))"""
    m = ref["planes"][0].numpy().astype(np.float64)
    if not o.obj_iou > 0:
        return m
    t = np.zeros_like(m)
    t[m == 1] = ((1.0 - o.obj_iou) + o.obj_iou * np.clip(values, 0.0, 1.0)).astype(np.float32).astype(np.float64)
    return t


def model(case, o, round_p=True, logits=None):
    """-> dict: conf, cls, grad (of lambda_conf conf + lambda_cls cls, float64 [N, A, 5 + C, h, w]), tobj.  logits: other logits for
    channels 4.. (with g > 0 the IoU values still come from the case's own, through box_loss_ref)"""
    ref = lc.reference(case)
    values = br.reference(case, o.box, o.lambda_box)["values"] if o.obj_iou > 0 else None
    tobj = _tobj(case, ref, o, values)
    s = _sig64(case, logits)
    conf, cls, g = _core(s.astype(np.float32).astype(np.float64) if round_p else s, case, ref, o, tobj)
    return dict(conf=conf, cls=cls, grad=g, tobj=tobj)


# ---- the cases ----

def _hyp_case(name, targets, why, tail=None):
    """a 4x6 map of the stride-16 head, 3 anchors, 3 classes, logits of set M; `tail(i) -> 1 + C values` replaces the confidence and class
    logits of positive cell i (None keeps the set-M value)"""
    N, T = targets.shape[:2]
    c = lc._case(name, 9000 + len(name), N, 3, 3, 4, 6, 64, 96, T, lc.ANC_LARGE, targets, why)
    if tail is not None:
        planes = lo.get_target(torch.from_numpy(c.targets), lo.scaled_anchors(c.anchors, (c.H, c.W), c.fh, c.fw), c.fw, c.fh, lc.THRES, c.C)
        x = c.logits.reshape(N, 3, 8, 4, 6)
        for i, (n, a, j, k) in enumerate(np.argwhere(planes[0].numpy() == 1)):
            for c5, v in enumerate(tail(i)):
                if v is not None:
                    x[n, a, 4 + c5, j, k] = np.float32(v)
    return c


def build_added():
    out = []
    out.append(_hyp_case("pos_noobj", br._rows([[(0.55, 0.45, 0.9, 0.9, 1)], [(0.3, 0.6, 0.95, 0.85, 2), (0.8, 0.2, 0.2, 0.3, 0)]], 2),
                         "targets so large that no anchor's IoU exceeds the ignore threshold: positive cells with noobj_mask = 1"))
    out.append(_hyp_case("multi_hot", br._rows([[(2.2 / 6, 1.7 / 4, 0.30, 0.45, 0), (2.6 / 6, 1.3 / 4, 0.32, 0.47, 2), (0.7, 0.8, 0.2, 0.2, 1)]]),
                         "two targets of classes 0 and 2 in one cell with one best anchor: a two-hot class plane"))
    s = [float(v) for v in lc.S_VALUES]
    rows = [[((k + 0.4) / 6, (n * 2 + 0.6) / 4, 0.2 + 0.03 * k, 0.35 - 0.03 * k, k % 3) for k in range(6)] for n in range(2)]
    out.append(_hyp_case("sat_pos", br._rows(rows, 2), "confidence and class logits of set S at every positive cell (one class logit per cell stays M): p exactly 0 or 1",
                         tail=lambda i: [None if c == 1 + i % 3 else s[(7 * i + 5 * c) % 12] for c in range(4)]))
    return out


_built = {}


def added_cases():
    if "added" not in _built:
        _built["added"] = build_added()
    return _built["added"]


def cases():
    return br.cases() + added_cases()


def judged_cases():
    return [c for c in cases() if c.logit_set != "band"]


def case_by_name(name):
    return {c.name: c for c in cases()}[name]


SUBSET = ("e17", "n130", "e3_S", "small_S", "nopos", "thres") + tuple(c.name for c in br.added_cases()) + ("pos_noobj", "multi_hot", "sat_pos")


# ---- model and twin of a case under an option set ----

_refs = {}


def reference(case, name, defect=None):
    """name: a key of OPTION_SETS or an Opts -> dict: opts, losses float64 [7] (total, then x y w h or box 0 0 0, conf, cls), grad float64
    like the logits, twin_losses float32 [7], twin_grad, kinds {name: bool mask [N, A, 5 + C, h, w]}, tobj, twin_tobj, counted, n_pos.
    Cached (without a defect).  With a defect: the float64 definition with the defect planted, in place of the model."""
    o = OPTION_SETS[name] if isinstance(name, str) else name
    key = (case.name, o)
    if defect is None and key in _refs:
        return _refs[key]
    base = lc.reference(case)
    shape5 = (case.N, case.A, 5 + case.C, case.fh, case.fw)
    if o.box is None:
        b = dict(losses=base["m64"]["losses"], grad=base["m64"]["grad"], twin_losses=base["twin_losses"], twin_grad=base["twin_grad"],
                 kinds=base["kinds"])
        part = 2.5 * (b["losses"][1] + b["losses"][2] + b["losses"][3] + b["losses"][4])
        tl = b["twin_losses"]
        tpart = F32(F32(F32(tl[1] * F32(2.5) + tl[2] * F32(2.5)) + tl[3] * F32(2.5)) + tl[4] * F32(2.5))
    else:
        b = br.reference(case, o.box, o.lambda_box)
        part = o.lambda_box * b["losses"][1]
        tpart = F32(o.lambda_box) * b["twin_losses"][1]
    if defect in (None, "gain_on_reported"):
        m = model(case, o)
    else:
        d = head_loss(case, o, torch.float64, defect, round_p=True)
        m = dict(conf=float(d["conf"]), cls=float(d["cls"]), grad=d["grad"].reshape(shape5), tobj=d["tobj"])
    losses = np.array([part + o.lambda_conf * m["conf"] + o.lambda_cls * m["cls"]] + list(b["losses"][1:5]) + [m["conf"], m["cls"]], np.float64)
    if defect == "gain_on_reported":
        losses[5], losses[6] = o.lambda_conf * m["conf"], o.lambda_cls * m["cls"]
    grad = m["grad"].reshape(shape5).copy()
    grad[:, :, 0:4] += np.asarray(b["grad"], np.float64).reshape(shape5)[:, :, 0:4]   # (iou_grad: the defect's own flow into the box logits stays)
    t = head_loss(case, o, torch.float32)
    ttotal = torch.tensor(tpart) + torch.tensor(o.lambda_conf, dtype=torch.float32) * t["conf"] + torch.tensor(o.lambda_cls, dtype=torch.float32) * t["cls"]
    twin_losses = np.array([float(ttotal)] + [float(v) for v in b["twin_losses"][1:5]] + [float(t["conf"]), float(t["cls"])], np.float32)
    twin_grad = t["grad"].reshape(shape5).copy()
    twin_grad[:, :, 0:4] = np.asarray(b["twin_grad"], np.float64).reshape(shape5)[:, :, 0:4]
    out = dict(opts=o, losses=losses, grad=grad, twin_losses=twin_losses, twin_grad=twin_grad, kinds=b["kinds"], tobj=m["tobj"],
               twin_tobj=t["tobj"], counted=base["counted"], n_pos=base["m64"]["n_pos"])
    if defect is None:
        _refs[key] = out
    return out


# ---- the comparator ----

def judge(case, name, losses8, grad=None, ref=None):
    """losses8: the eight float32 of d_losses; grad like the logits or None -> loss_cases.Report"""
    ref = ref or reference(case, name)
    o = ref["opts"]
    rep = lc.Report(case)
    if float(losses8[7]) != float(ref["counted"]):
        rep.failures.append("%s losses[7] = %r, want %d" % (case.name, float(losses8[7]), ref["counted"]))
    if o.box is not None and any(float(losses8[i]) != 0.0 for i in (2, 3, 4)):
        rep.failures.append("%s losses[2..4] = %r, want exact zeros" % (case.name, [float(v) for v in losses8[2:5]]))
    if case.logit_set == "band":
        fin = [math.isfinite(float(v)) for v in losses8[:7]]
        ok = all(fin[1:6]) and (fin[0] and fin[6]) != (ref["n_pos"] == 0) and (grad is None or bool(np.isfinite(grad).all()))
        if not ok:
            rep.failures.append("%s: a loss or gradient of the band case is not finite (or not the documented NaN): %r" % (case.name, list(losses8)))
        return rep
    names = lo.LOSS_NAMES if o.box is None else ("total", "box", None, None, None, "conf", "cls")
    for i, nm in enumerate(names):
        if nm is None:
            continue
        d, w, t = float(losses8[i]), float(ref["losses"][i]), float(ref["twin_losses"][i])
        if math.isnan(w):
            rep.add("loss " + nm, float("nan"), float("nan"), float("nan"), math.isnan(d))
            continue
        bound = max(lc.ACCURACY_RATIO * abs(t - w), lc.LOSS_ULPS * lc.ulp32(w))
        rep.add("loss " + nm, abs(d - w), abs(t - w), bound, math.isfinite(d) and abs(d - w) <= bound)
    if grad is None:
        return rep
    if not np.isfinite(grad).all():
        rep.failures.append("%s: a gradient element is not finite" % case.name)
    shape = next(iter(ref["kinds"].values())).shape
    g, w, t = (np.asarray(a, np.float64).reshape(shape) for a in (grad, ref["grad"], ref["twin_grad"]))
    for nm, sel in ref["kinds"].items():
        if not sel.any() or (nm == "box" and case.name in BOX_TIES):
            continue
        top = np.abs(w[sel]).max()
        if nm in ALWAYS_ZERO:
            rep.add("grad " + nm, float(np.abs(np.nan_to_num(g[sel], nan=np.inf)).max()), float(np.abs(t[sel]).max()), 0.0, bool(top == 0 and (g[sel] == 0).all()))
            continue
        d, dt = np.abs(g[sel] - w[sel]).max(), np.abs(t[sel] - w[sel]).max()
        bound = max(lc.ACCURACY_RATIO * dt, lc.GRAD_ULPS * lc.ulp32(top))
        rep.add("grad " + nm, float(d), float(dt), bound, bool(np.isfinite(g[sel]).all() and d <= bound))
    return rep


Q_STEP = 2.0 ** -24          # float32's spacing just below 1: what the twin's 1 - p_t is a multiple of


def twin_condition(case, name, widened=True):
    """[failures]: conf, cls and the kinds conf_pos, conf_noobj, cls of the twin against the model within the ulp floors alone plus what the
    number format itself is worth to the model: SIGMOID_ULPS float32 steps of every sigmoid (loss_cases.py explains why); under focal one
    Q_STEP of 1 - p_t, which float32 forms as a multiple of 2^-24 (at p = 2e-9 and t = 0 it is 0 in float32 and 2e-9 in float64); and with
    g > 0 what the twin's own float32 IoU values move t_obj by.  For a loss: the sum over its elements of the larger change.
    The last two are a widening of loss_cases.twin_condition; widened=False leaves them out (test_cpu_loss_hyp.py pins what then fails:
    a8c20 and thres by a few per cent of one gradient floor, and sat_pos, all under `all` / `all_ref`, which the table must keep)."""
    ref = reference(case, name)
    o = ref["opts"]
    base = lc.reference(case)
    s32 = _sig64(case).astype(np.float32)
    s64 = s32.astype(np.float64)
    p0 = {}
    _, _, g = _core(s64, case, base, o, ref["tobj"], parts=p0)
    free = (s32 > 0) & (s32 < 1)

    def change(sig, tobj, dq=0.0):
        p1 = {}
        _, _, g1 = _core(sig, case, base, o, tobj, dq, parts=p1)
        return np.array([np.abs(p1[k] - p0[k]).sum() for k in ("conf", "cls")]), np.abs(g1 - g)
    al, ag = np.zeros(2), np.zeros_like(g)
    for toward in (F32(2), F32(-1)):
        dl, dg = change(np.where(free, np.nextafter(s32, toward), s32).astype(np.float64), ref["tobj"])
        al, ag = np.maximum(al, lc.SIGMOID_ULPS * dl), np.maximum(ag, lc.SIGMOID_ULPS * dg)
    if o.fl_gamma > 0 and widened:
        ql, qg = np.zeros(2), np.zeros_like(g)
        for dq in (Q_STEP, -Q_STEP):
            dl, dg = change(s64, ref["tobj"], dq)
            ql, qg = np.maximum(ql, dl), np.maximum(qg, dg)
        al, ag = al + ql, ag + qg
    if o.obj_iou > 0 and widened:
        dl, dg = change(s64, ref["twin_tobj"])
        al, ag = al + dl, ag + dg
    out = []
    for i, (idx, nm) in enumerate(((5, "conf"), (6, "cls"))):
        w, t = float(ref["losses"][idx]), float(ref["twin_losses"][idx])
        if math.isnan(w) != math.isnan(t) or (not math.isnan(w) and abs(t - w) > lc.LOSS_ULPS * lc.ulp32(w) + al[i]):
            out.append("%s loss %s: twin %r, model %r, allowed %.3e" % (case.name, nm, t, w, lc.LOSS_ULPS * lc.ulp32(w) + al[i]))
    shape = g.shape
    tg, wg = ref["twin_grad"].reshape(shape), ref["grad"].reshape(shape)
    for nm in ("conf_pos", "conf_noobj", "cls"):
        sel = ref["kinds"][nm]
        if not sel.any():
            continue
        top = np.abs(wg[sel]).max()
        over = np.abs(tg[sel] - wg[sel]) - (lc.GRAD_ULPS * lc.ulp32(top) + ag[sel]) if top > 0 else np.abs(tg[sel])
        if over.max() > 0:
            out.append("%s grad %s: twin off by %.3e beyond what is allowed (kind's maximum %.3e)" % (case.name, nm, over.max(), top))
    return out
