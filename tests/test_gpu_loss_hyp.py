"""yolov5's objectness / class loss options of one head on the device -- loss_cells_kernel<GRAD, BOX, true> and loss_final_kernel
(csrc/yf_loss_kernels.hip, csrc/yf_loss_term.h) behind yf_train_head_loss_hyp_workspace_bytes / yf_train_head_loss_hyp, called through
ctypes -- against the float64 model of tests/loss_hyp_ref.py (its docstring states the definition, the option sets, the cases and the
comparator; tests/test_cpu_loss_hyp.py shows on the CPU that the definition is yolov5's, that the model's closed-form gradient is float64
autograd's, that the cases have their properties and that the comparator rejects every planted defect).

Per run: the workspace is exactly the box entry's size; it, d_losses[8] and d_grad_head sit between two 4 KiB guards of 0xA5 bytes that
must come back untouched; the gradient is pre-filled with a NaN pattern and must come back fully written; the 8 + C planes are bit for
bit those yf_train_head_loss_box leaves (smoothing and the IoU target are applied where the planes are read, never stored); d_losses is
recomputed exactly from the 16 doubles.

MEASURED (MI355X; per option set and judged quantity the worst case of the table: distance to the model / the bound it is held to, then
the case, the device's and the twin's distance and which side of the max() the bound is; test_measured_worst_ratio prints it; no bound
comes from it; the sets `all`, `all_ref`, `gamma1.5` and `gr_giou` here, every set in DESIGN.md section 6, "yolov5's objectness and class
options"):
  gamma1.5    loss total      0.42  pred_inside   device 6.03e-07  twin 4.84e-07  3 x twin
  gamma1.5    loss conf       0.38  disjoint      device 2.50e-07  twin 2.20e-07  3 x twin
  gamma1.5    loss cls        0.30  multi_hot     device 1.18e-06  twin 1.30e-06  3 x twin
  gamma1.5    grad conf_pos   0.43  small_S       device 1.53e-10  twin 1.19e-10  3 x twin
  gamma1.5    grad conf_noobj 0.33  small_S       device 2.92e-10  twin 2.92e-10  3 x twin
  gamma1.5    grad cls        0.36  thres         device 7.99e-10  twin 7.46e-10  3 x twin
  gr_giou     loss total      0.44  thres         device 8.31e-07  twin 5.93e-07  ulp floor
  gr_giou     loss conf       0.41  nopos         device 1.97e-07  twin 1.37e-07  ulp floor
  gr_giou     loss cls        0.33  multi_hot     device 1.52e-06  twin 1.52e-06  3 x twin
  gr_giou     grad conf_pos   0.25  clamp         device 4.66e-10  twin 4.66e-10  ulp floor
  gr_giou     grad conf_noobj 0.29  pos_noobj     device 3.10e-10  twin 3.62e-10  3 x twin
  gr_giou     grad cls        0.53  pos_noobj     device 1.57e-08  twin 9.11e-09  ulp floor
  all         loss total      0.58  counted       device 1.39e-07  twin 7.90e-08  ulp floor
  all         loss conf       0.44  a8c20         device 1.21e-07  twin 9.15e-08  3 x twin
  all         loss cls        0.46  a8c20         device 4.41e-07  twin 3.22e-07  3 x twin
  all         grad conf_pos   0.82  cell_same_S   device 9.49e-11  twin 2.15e-11  ulp floor
  all         grad conf_noobj 0.46  a8c20         device 4.30e-10  twin 3.14e-10  3 x twin
  all         grad cls        0.73  e257          device 6.45e-09  twin 2.97e-09  3 x twin
  all_ref     loss total      0.38  pred_inside   device 3.62e-07  twin 2.43e-07  ulp floor
  all_ref     loss conf       0.52  e255          device 1.23e-07  twin 6.38e-08  ulp floor
  all_ref     loss cls        0.46  a8c20         device 4.41e-07  twin 3.22e-07  3 x twin
  all_ref     grad conf_pos   0.45  small         device 1.29e-10  twin 9.59e-11  3 x twin
  all_ref     grad conf_noobj 0.46  a8c20         device 4.30e-10  twin 3.14e-10  3 x twin
  all_ref     grad cls        0.73  e257          device 6.45e-09  twin 2.97e-09  3 x twin
The whole file (127 tests) takes 6.6 s on one MI355X.
"""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import box_loss_ref as br  # noqa: E402
import loss_cases as lc  # noqa: E402
import loss_hyp_ref as hr  # noqa: E402
import loss_run as lr  # noqa: E402

CASES = hr.cases()
SUBSET = [hr.case_by_name(n) for n in hr.SUBSET]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from yolo_fastest_amd import _lib
    return _lib.lib()


def _kind(o):
    return br.KIND_ID[o.box] if o.box else 0


def run(lib, dev, c, o, grad=True, stream=None):
    """o: loss_hyp_ref.Opts"""
    return lr.run(lib, dev, c, "hyp", kind=_kind(o), lam=o.lambda_box, opts=o[:8], grad=grad, stream=stream)


_results, _box = {}, {}


def _result(lib, dev, c, name):
    if (c.name, name) not in _results:
        _results[c.name, name] = run(lib, dev, c, hr.OPTION_SETS[name])
    return _results[c.name, name]


def _box_result(lib, dev, c, kind):
    """yf_train_head_loss_box on the same inputs, once per case and box_kind"""
    if (c.name, kind) not in _box:
        _box[c.name, kind] = lr.run(lib, dev, c, "box", kind=kind, lam=br.LAMBDA_BOX)
    return _box[c.name, kind]


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _check_acc(c, o, acc, l8):
    """d_losses is loss_final_kernel's float32 arithmetic on exactly the workspace's 16 doubles"""
    F = np.float32
    E = float(c.N * c.A * c.fh * c.fw)
    ref = lc.reference(c)
    assert acc[7] == ref["m64"]["n_pos"] and acc[8] == ref["counted"] and (acc[9:] == 0).all(), (c.name, acc)
    with np.errstate(invalid="ignore", divide="ignore"):
        l = [F(acc[i] / E) for i in range(4)]
        lconf = F(F(acc[4] / E) + F(0.5) * F(acc[5] / E))
        lcls = F(acc[6] / (c.C * acc[7]))
        tail = (lconf * F(o.lambda_conf), lcls * F(o.lambda_cls))
        if o.box:
            assert (acc[1:4] == 0).all()
            total = F(F(F(o.lambda_box) * l[0] + tail[0]) + tail[1])
            want = [total, l[0], 0, 0, 0]
        else:
            total = F(F(F(F(F(l[0] * F(2.5) + l[1] * F(2.5)) + l[2] * F(2.5)) + l[3] * F(2.5)) + tail[0]) + tail[1])
            want = [total] + l
    want = np.array(want + [lconf, lcls, acc[8]], np.float32)
    assert np.array_equal(want, l8, equal_nan=True), (c.name, want, l8)


def _judge(lib, dev, c, name, l8, g, dense, acc):
    o = hr.OPTION_SETS[name]
    rep = hr.judge(c, name, l8, g)
    _check_acc(c, o, acc, l8)
    if not np.array_equal(_bits(dense), _bits(_box_result(lib, dev, c, _kind(o))[2])):
        rep.failures.append("%s: the planes differ from yf_train_head_loss_box's" % c.name)
    return rep


@pytest.mark.parametrize("name", ["all", "all_ref"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_case_against_the_float64_model(lib, dev, capsys, case, name):
    l8, g, dense, acc = _result(lib, dev, case, name)
    rep = _judge(lib, dev, case, name, l8, g, dense, acc)
    with capsys.disabled():
        print("\n" + name + " " + rep.table())
    assert rep.ok, "\n".join(rep.failures)


@pytest.mark.parametrize("name", hr.SINGLE_KNOB)
def test_every_single_knob_on_the_subset(lib, dev, capsys, name):
    bad, lines = [], []
    for c in SUBSET:
        l8, g, dense, acc = _result(lib, dev, c, name)
        rep = _judge(lib, dev, c, name, l8, g, dense, acc)
        lines.append(name + " " + rep.table())
        bad += rep.failures
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert not bad, "\n".join(bad)


def test_whole_table_without_the_gradient(lib, dev):
    """d_grad_head = NULL: the same planes, counter and losses"""
    bad = []
    for name in ("all", "all_ref"):
        for c in CASES:
            l8, g, dense, acc = run(lib, dev, c, hr.OPTION_SETS[name], grad=False)
            bad += _judge(lib, dev, c, name, l8, None, dense, acc).failures
    assert not bad, "\n".join(bad)


NEUTRALS = (hr.NEUTRAL, hr.opts(fl_alpha=0.9))                 # fl_alpha is not read while gamma is 0


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_neutral_options_are_the_box_entry_bit_for_bit(lib, dev, kind):
    """losses, gradient and the whole workspace; the sums are double atomicAdds whose order differs from run to run, so acc[0..6] are held
    to 1e-12 relative and the seven losses to one float32 ulp (as test_gpu_box_loss.py holds two runs of one entry), everything else to the
    bit"""
    box = {v: k for k, v in br.KIND_ID.items()}.get(kind)
    for o in NEUTRALS:
        for c in CASES:
            l8, g, dense, acc = run(lib, dev, c, o._replace(box=box))
            bl8, bg, bdense, bacc = _box_result(lib, dev, c, kind)
            assert np.array_equal(_bits(g), _bits(bg)), c.name
            assert np.array_equal(_bits(dense), _bits(bdense)), c.name
            assert np.array_equal(acc[7:], bacc[7:]) and l8[7] == bl8[7], c.name
            assert np.allclose(acc[:7], bacc[:7], rtol=1e-12, atol=0), (c.name, acc, bacc)
            for a, b in zip(l8[:7], bl8[:7]):
                a, b = float(a), float(b)
                assert (math.isnan(a) and math.isnan(b)) or abs(a - b) <= lc.ulp32(b), (c.name, a, b)
            if kind == 0:
                el8, eg, edense, _ = lr.run(lib, dev, c, "ex")
                assert np.array_equal(_bits(g), _bits(eg)) and np.array_equal(_bits(dense[:6 + c.C]), _bits(edense)), c.name


@pytest.mark.parametrize("kind", [0, 3])
def test_a_gain_of_two_doubles_its_channels_bits_and_no_others(lib, dev, kind):
    box = {v: k for k, v in br.KIND_ID.items()}.get(kind)
    for c in SUBSET:
        if c.logit_set == "band":
            continue
        bl8, bg, _, _ = _box_result(lib, dev, c, kind)
        s5 = (c.N, c.A, 5 + c.C, c.fh, c.fw)
        bg = bg.reshape(s5)
        for o, doubled in ((hr.opts(lambda_conf=2.0, box=box), slice(4, 5)), (hr.opts(lambda_cls=2.0, box=box), slice(5, None))):
            l8, g, _, _ = run(lib, dev, c, o)
            want = bg.copy()
            want[:, :, doubled] = np.float32(2) * want[:, :, doubled]
            assert np.array_equal(_bits(g.reshape(s5)), _bits(want)), (c.name, o)
            for i in (5, 6):                                    # the reported conf and cls stay unweighted
                a, b = float(l8[i]), float(bl8[i])
                assert (math.isnan(a) and math.isnan(b)) or abs(a - b) <= lc.ulp32(b), (c.name, i, a, b)


@pytest.mark.parametrize("name", ["all", "all_ref", "gamma2"])
@pytest.mark.parametrize("case", ["large", "n130", "small_S", "thres"])
def test_two_runs_give_the_same_gradient_bits_and_sums_within_one_ulp(lib, dev, case, name):
    c = hr.case_by_name(case)
    assert c.N * c.A * c.fh * c.fw > 256                    # more than one workgroup adds to each sum
    a, b = run(lib, dev, c, hr.OPTION_SETS[name]), run(lib, dev, c, hr.OPTION_SETS[name])
    assert np.array_equal(_bits(a[1]), _bits(b[1]))
    assert np.array_equal(_bits(a[2]), _bits(b[2]))
    for i in range(7):
        assert abs(float(a[0][i]) - float(b[0][i])) <= lc.ulp32(a[0][i]), (i, a[0][i], b[0][i])
    assert a[0][7] == b[0][7] == 0


@pytest.mark.parametrize("case", ["e17", "n130", "thres_S", "nopos", "sat_pos"])
def test_on_a_stream_of_its_own(lib, dev, case):
    c = hr.case_by_name(case)
    s = torch.cuda.Stream(dev)
    assert s.cuda_stream != torch.cuda.current_stream(dev).cuda_stream
    l8, g, dense, acc = run(lib, dev, c, hr.OPTION_SETS["all"], stream=s)
    rep = _judge(lib, dev, c, "all", l8, g, dense, acc)
    assert rep.ok, "\n".join(rep.failures)
    assert np.array_equal(_bits(g), _bits(_result(lib, dev, c, "all")[1]))


def test_refusals(lib, dev):
    from yolo_fastest_amd import _lib
    c = hr.case_by_name("e17")
    need = lr.need(lib, c, "hyp")
    n = ctypes.c_size_t()
    assert lib.yf_train_head_loss_hyp_workspace_bytes(c.N, c.fh, c.fw, 9, c.C, ctypes.byref(n)) == _lib.YF_E_INVALID
    assert lib.yf_train_head_loss_hyp_workspace_bytes(c.N, c.fh, c.fw, c.A, c.C, None) == _lib.YF_E_INVALID
    x, t = torch.from_numpy(c.logits).to(dev), torch.from_numpy(c.targets).to(dev)
    work, losses, grad = lr.Guarded(need + 8, dev), lr.Guarded(32, dev), lr.Guarded(c.logits.size * 4, dev)

    def call(o=hr.OPTION_SETS["all"], kind=None, lam=br.LAMBDA_BOX, ptr=work.ptr, nbytes=need, T=c.T):
        return lr.call(lib, "hyp", c, x, t, ptr, nbytes, losses.ptr, grad.ptr, None, _kind(o) if kind is None else kind, lam, o[:8], T=T)
    nan, inf = float("nan"), float("inf")
    ok = hr.OPTION_SETS["all"]
    refused = [ok._replace(**{f: v}) for f in hr.OPTION_NAMES for v in (nan, inf, -inf)]
    refused += [ok._replace(obj_pw=0.0), ok._replace(obj_pw=-1.0), ok._replace(cls_pw=0.0), ok._replace(cls_pw=-2.0),
                ok._replace(label_smoothing=-0.01), ok._replace(label_smoothing=1.01), ok._replace(fl_gamma=-1.0), ok._replace(fl_gamma=0.5),
                ok._replace(fl_gamma=1e-9), ok._replace(fl_gamma=0.999), ok._replace(fl_alpha=-0.1), ok._replace(fl_alpha=1.1),
                ok._replace(obj_iou=-0.1), ok._replace(obj_iou=1.1), ok._replace(lambda_conf=-1e-300), ok._replace(lambda_cls=-1.0),
                hr.opts(fl_alpha=2.0), hr.opts(fl_alpha=nan)]                       # (refused although gamma = 0 leaves alpha unread)
    for o in refused:
        assert call(o) == _lib.YF_E_INVALID, o
    assert call(ok, kind=0) == _lib.YF_E_INVALID and b"obj_iou" in lib.yf_last_error_string()     # g > 0 with YF_BOX_REF
    assert call(hr.opts(obj_iou=1e-6)) == _lib.YF_E_INVALID
    for kind in (-1, 4):
        assert call(kind=kind) == _lib.YF_E_INVALID and b"box_kind" in lib.yf_last_error_string()
    for lam in (-1.0, nan, inf):
        assert call(lam=lam) == _lib.YF_E_INVALID and b"lambda_box" in lib.yf_last_error_string()
    assert call(T=0) == _lib.YF_E_INVALID
    assert call(nbytes=need - 1) == _lib.YF_E_WORKSPACE
    assert call(nbytes=lr.need(lib, c, "ex")) == _lib.YF_E_WORKSPACE          # yf_train_head_loss_ex's size is two planes short
    assert call(ptr=work.ptr + 4) == _lib.YF_E_INVALID and b"aligned" in lib.yf_last_error_string()
    torch.cuda.synchronize(dev)
    assert (work.buf == 0xA5).all() and (losses.buf == 0xA5).all() and (grad.buf == 0xA5).all()      # a refused call launches nothing
    for o in (ok, hr.OPTION_SETS["all_ref"], hr.opts(fl_gamma=1.0), hr.opts(label_smoothing=1.0), hr.opts(lambda_conf=0.0, lambda_cls=0.0),
              hr.opts(obj_iou=1.0, box="giou"), hr.NEUTRAL):
        assert call(o) == 0, o
    torch.cuda.synchronize(dev)
    assert work.guards_untouched() and losses.guards_untouched() and grad.guards_untouched()


def _kwargs(o):
    return dict(zip(hr.OPTION_NAMES, o[:8]), box_loss=o.box, lambda_box=o.lambda_box)


def test_through_YOLOLossV3(lib, dev):
    """validation.YOLOLossV3(..., the options)(pred, targets): the C entry's numbers; the gradient scales through backward(); and with the
    defaults still yf_train_head_loss_ex bit for bit, as before"""
    from yolo_fastest_amd import validation as val
    c = hr.case_by_name("small")
    t = torch.from_numpy(c.targets).to(dev)
    for name in ("all", "all_ref", "gamma2", "gr_giou", "lambda_conf"):
        o = hr.OPTION_SETS[name]
        l8, g, _, _ = _result(lib, dev, c, name)
        crit = val.YOLOLossV3(c.anchors, c.C, [c.H, c.W, 1], dev, **_kwargs(o))
        x = torch.from_numpy(c.logits).to(dev).requires_grad_(True)
        out = crit(x, t)
        assert len(out) == 7
        got = np.array([out[0].item()] + list(out[1:]) + [0.0], np.float32)
        assert hr.judge(c, name, got).ok
        for i in range(7):
            assert abs(float(got[i]) - float(l8[i])) <= lc.ulp32(l8[i])
        (3.0 * out[0]).backward()
        assert torch.equal(x.grad.cpu(), 3.0 * torch.from_numpy(g))
    # the defaults: yf_train_head_loss_ex, and with box_loss alone yf_train_head_loss_box
    default = val.YOLOLossV3(c.anchors, c.C, [c.H, c.W, 1], dev)                  # default-constructed: the parent's call, the parent's bits
    for crit, want in ((default, lr.run(lib, dev, c, "ex")),
                       (val.YOLOLossV3(c.anchors, c.C, [c.H, c.W, 1], dev, fl_alpha=0.9), lr.run(lib, dev, c, "ex")),
                       (val.YOLOLossV3(c.anchors, c.C, [c.H, c.W, 1], dev, box_loss="ciou"), _box_result(lib, dev, c, 3)),
                       (val.YOLOLossV3(c.anchors, c.C, [c.H, c.W, 1], dev, box_loss="ciou", fl_alpha=0.9), _box_result(lib, dev, c, 3))):
        x = torch.from_numpy(c.logits).to(dev).requires_grad_(True)
        out = crit(x, t)
        out[0].backward()
        assert np.array_equal(_bits(x.grad.cpu().numpy()), _bits(want[1]))
        assert all(abs(float(a) - float(b)) <= lc.ulp32(b) for a, b in zip([out[0].item()] + list(out[1:]), want[0][:7]))


def test_one_train_step_with_loss_hyp_ciou_and_ema(dev):
    import yolo_fastest_amd as yf
    from yolo_fastest_amd import training, validation as val
    io = yf.io_params_for(256)
    torch.manual_seed(3)
    m = yf.YoloFastest(io)
    m.initialize_weights()
    m = m.to(dev).train()
    x = (torch.rand(4, 1, 64, 96, generator=torch.Generator().manual_seed(1)) - 0.5).to(dev)
    t = np.zeros((4, 8, 6), np.float32)
    t[:, 0] = (0.4, 0.6, 0.3, 0.2, 1, 255.0)
    t[:, 1] = (0.7, 0.3, 0.5, 0.6, 2, 255.0)
    loss_hyp = {"obj": 0.7, "cls": 1.3, "obj_pw": 1.7, "cls_pw": 0.6, "fl_gamma": 1.5, "fl_alpha": 0.3, "label_smoothing": 0.1, "gr": 1.0}
    kw = {training.LOSS_HYP_KEYS[k]: v for k, v in loss_hyp.items()}
    crit = [val.YOLOLossV3(io["anchors"][i], 3, [64, 96, 1], dev, model=m, box_loss="ciou", **kw) for i in range(2)]
    before = [p.detach().clone() for p in m.parameters()]
    ema = training.ModelEMA(m)
    losses = training.train_step(m, crit, training.Adam(m.parameters(), lr=1e-3), x, torch.from_numpy(t).to(dev), [0.5, 1.5], ema=ema)
    assert all(math.isfinite(float(v)) for v in losses)
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters()) and all(bool(torch.isfinite(p).all()) for p in ema.ema.parameters())
    assert any(not torch.equal(a, b) for a, b in zip(before, m.parameters()))


def test_measured_worst_ratio(lib, dev, capsys):
    """prints the MEASURED table: per option set and judged quantity, over the judged cases it ran on, the worst distance / bound, the case,
    and the device's and the twin's distances"""
    lines, ok = [], True
    for name in hr.OPTION_SETS:
        worst = {}
        for c in (CASES if name.startswith("all") else SUBSET):
            if c.logit_set == "band":
                continue
            l8, g, _, _ = _result(lib, dev, c, name)
            for what, d, tw, bound in hr.judge(c, name, l8, g).rows:
                if not math.isnan(d) and bound > 0:
                    r = d / bound
                    if what not in worst or r > worst[what][0]:
                        worst[what] = (r, c.name, d, tw, "ulp floor" if bound > lc.ACCURACY_RATIO * tw else "3 x twin")
        for what, (r, cname, d, tw, which) in worst.items():
            if what in ("loss total", "loss conf", "loss cls", "grad conf_pos", "grad conf_noobj", "grad cls"):
                lines.append("  %-11s %-15s %.2f  %-13s device %.2e  twin %.2e  %s" % (name, what, r, cname, d, tw, which))
            ok = ok and r <= 1
    with capsys.disabled():
        print("\n[loss options: worst distance / bound per option set]\n" + "\n".join(lines))
    assert ok
