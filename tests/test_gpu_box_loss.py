"""The IoU-family box loss of one head on the device -- loss_targets_kernel's gw / gh planes, loss_cells_kernel<GRAD, true>,
loss_final_kernel's box branch (csrc/yf_loss_kernels.hip, csrc/yf_box_term.h) behind yf_train_head_loss_box_workspace_bytes /
yf_train_head_loss_box, called through ctypes -- against the float64 autograd model of tests/box_loss_ref.py (its docstring states the
definition, the cases and the comparator; tests/test_cpu_box_loss.py shows on the CPU that the cases have their properties, that the
kernel's per-cell function matches the model when compiled for the host, and that the comparator rejects every planted defect).

Per case and kind: the workspace is exactly the reported size; it, d_losses[8] and d_grad_head sit between two 4 KiB guards of 0xA5
bytes that must come back untouched (tests/loss_run.py, the one runner); the gradient is pre-filled with a NaN pattern and must come back
fully written.  The first 6 + C planes are bit for bit those yf_train_head_loss_ex leaves for the same inputs (and get_target's, by
loss_cases.judge_planes); gw and gh bit for bit box_loss_ref.size_planes.  d_losses is recomputed exactly from the 16 doubles.  Losses
and the `box` gradient are held to max(3 x the twin's distance, the ulp floor); box_off is exactly zero; the gradient of channels 4.. is
bit-identical to yf_train_head_loss_ex's and conf / cls within one float32 ulp of it (their double sums are atomicAdds, whose order
differs from run to run).  box_kind 0 is yf_train_head_loss_ex.

MEASURED (MI355X; per kind of box loss and per judged quantity the worst case of the table: distance to the model / the bound it is
held to, then the case, the device's and the twin's distance and which side of the max() the bound is;
test_measured_worst_ratio_per_kind prints it; no bound comes from it):
  giou  loss total  0.55  a8c20         device 1.04e-06  twin 5.66e-07  ulp floor
  giou  loss box    0.06  e3            device 2.91e-08  twin 2.91e-08  ulp floor
  giou  grad box    0.12  last_wins     device 1.86e-09  twin 4.82e-09  ulp floor
  diou  loss total  0.45  thres         device 8.55e-07  twin 6.16e-07  ulp floor
  diou  loss box    0.06  cell_diff     device 1.83e-09  twin 1.89e-09  ulp floor
  diou  grad box    0.11  pred_inside   device 2.10e-10  twin 6.22e-10  3 x twin
  ciou  loss total  0.45  thres         device 9.05e-07  twin 6.67e-07  3 x twin
  ciou  loss box    0.06  e16           device 7.34e-09  twin 7.56e-09  ulp floor
  ciou  grad box    0.12  aspect        device 4.45e-10  twin 4.45e-10  ulp floor
  (a `grad box` ratio of 0.12 against a 4-ulp floor is half an ulp, the store's own rounding: the term is evaluated in double.)
  box_off exactly zero, the planes identical and the gradient of channels 4.. bit-identical to yf_train_head_loss_ex's in every case.
The whole file (146 tests) takes 4.9 s on one MI355X.
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
import loss_run as lr  # noqa: E402
import test_gpu_loss as tg  # noqa: E402  (_check_acc: box_kind 0 is held to loss_final_kernel's arithmetic without a box)

CASES = br.cases()
LAM = br.LAMBDA_BOX


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from yolo_fastest_amd import _lib
    return _lib.lib()


def run(lib, dev, c, kind, lam=LAM, grad=True, stream=None):
    """kind: 0 .. 3"""
    return lr.run(lib, dev, c, "box", kind=kind, lam=lam, grad=grad, stream=stream)


_results, _ex = {}, {}


def _result(lib, dev, c, kind):
    if (c.name, kind) not in _results:
        _results[c.name, kind] = run(lib, dev, c, br.KIND_ID[kind])
    return _results[c.name, kind]


def _ex_result(lib, dev, c):
    """yf_train_head_loss_ex on the same inputs, once per case"""
    if c.name not in _ex:
        _ex[c.name] = lr.run(lib, dev, c, "ex")
    return _ex[c.name]


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _check_acc(c, acc, l8, ref, lam=LAM):
    """the workspace's 16 doubles as the header states them: d_losses is loss_final_kernel's float32 arithmetic (its box branch, both gains 1) on exactly these"""
    F = np.float32
    E = float(c.N * c.A * c.fh * c.fw)
    assert acc[7] == ref["n_pos"] and acc[8] == ref["counted"] and (acc[1:4] == 0).all() and (acc[9:] == 0).all(), (c.name, acc)
    with np.errstate(invalid="ignore", divide="ignore"):
        lbox = F(acc[0] / E)
        lconf = F(F(acc[4] / E) + F(0.5) * F(acc[5] / E))
        lcls = F(acc[6] / (c.C * acc[7]))
        total = F(F(F(lam) * lbox + lconf) + lcls)
    want = np.array([total, lbox, 0, 0, 0, lconf, lcls, acc[8]], np.float32)
    assert np.array_equal(want, l8, equal_nan=True), (c.name, want, l8)


def _check_against_ex(c, l8, g, dense, ex):
    """what the box loss must leave alone: the first 6 + C planes and the gradient of channels 4.. bit for bit, conf / cls within one ulp"""
    el8, eg, edense, _ = ex
    assert np.array_equal(_bits(dense[:6 + c.C]), _bits(edense)), (c.name, "the first 6 + C planes differ from yf_train_head_loss_ex's")
    for i in (5, 6):
        a, b = float(l8[i]), float(el8[i])
        assert (math.isnan(a) and math.isnan(b)) or abs(a - b) <= lc.ulp32(b), (c.name, i, a, b)
    if g is not None:
        s5 = (c.N, c.A, 5 + c.C, c.fh, c.fw)
        assert np.array_equal(_bits(g.reshape(s5)[:, :, 4:]), _bits(eg.reshape(s5)[:, :, 4:])), (c.name, "the gradient of channels 4.. differs")


def _judge(c, kind, l8, g, dense):
    rep = br.judge(c, kind, l8, g)
    lc.judge_planes(rep, dense[:6 + c.C], lc.reference(c)["planes"])
    want = br.planes_to_dense(c)
    for p, name in ((6 + c.C, "gw"), (7 + c.C, "gh")):
        if not np.array_equal(_bits(dense[p]), _bits(want[p])):
            rep.failures.append("%s plane %s differs" % (c.name, name))
    return rep


@pytest.mark.parametrize("kind", br.KINDS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_case_against_the_float64_model(lib, dev, capsys, case, kind):
    l8, g, dense, acc = _result(lib, dev, case, kind)
    rep = _judge(case, kind, l8, g, dense)
    with capsys.disabled():
        print("\n" + kind + " " + rep.table())
    _check_acc(case, acc, l8, br.reference(case, kind))
    _check_against_ex(case, l8, g, dense, _ex_result(lib, dev, case))
    assert rep.ok, "\n".join(rep.failures)


def test_box_kind_0_is_yf_train_head_loss_ex(lib, dev):
    for c in CASES:
        l8, g, dense, acc = run(lib, dev, c, 0, lam=7.0)            # (lambda_box is not read)
        el8, eg, edense, eacc = _ex_result(lib, dev, c)
        assert np.array_equal(_bits(g), _bits(eg)), c.name
        assert np.array_equal(_bits(dense[:6 + c.C]), _bits(edense)) and np.array_equal(_bits(dense[6 + c.C:]), _bits(br.planes_to_dense(c)[6 + c.C:])), c.name
        tg._check_acc(c, acc, l8, lc.reference(c))
        for i in range(7):                                          # the sums are double atomicAdds: one float32 ulp from run to run
            a, b = float(l8[i]), float(el8[i])
            assert (math.isnan(a) and math.isnan(b)) or abs(a - b) <= lc.ulp32(b), (c.name, i, a, b)
        assert l8[7] == el8[7]


def test_whole_table_without_the_gradient(lib, dev):
    """d_grad_head = NULL: the same planes, counter and losses"""
    bad = []
    for kind in br.KINDS:
        for c in CASES:
            l8, g, dense, acc = run(lib, dev, c, br.KIND_ID[kind], grad=False)
            bad += _judge(c, kind, l8, None, dense).failures
            _check_acc(c, acc, l8, br.reference(c, kind))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", ["e17", "n130", "thres_S", "nopos", "clamp"])
def test_on_a_stream_of_its_own(lib, dev, name):
    c = br.case_by_name(name)
    s = torch.cuda.Stream(dev)
    assert s.cuda_stream != torch.cuda.current_stream(dev).cuda_stream
    l8, g, dense, _ = run(lib, dev, c, br.KIND_ID["ciou"], stream=s)
    rep = _judge(c, "ciou", l8, g, dense)
    assert rep.ok, "\n".join(rep.failures)
    assert np.array_equal(_bits(g), _bits(_result(lib, dev, c, "ciou")[1]))


@pytest.mark.parametrize("kind", br.KINDS)
@pytest.mark.parametrize("name", ["large", "n130", "small_S", "thres"])
def test_two_runs_give_the_same_gradient_bits_and_sums_within_one_ulp(lib, dev, name, kind):
    c = br.case_by_name(name)
    assert c.N * c.A * c.fh * c.fw > 256                    # more than one workgroup adds to each sum
    a, b = run(lib, dev, c, br.KIND_ID[kind]), run(lib, dev, c, br.KIND_ID[kind])
    assert np.array_equal(_bits(a[1]), _bits(b[1]))
    assert np.array_equal(_bits(a[2]), _bits(b[2]))
    for i in range(7):
        assert abs(float(a[0][i]) - float(b[0][i])) <= lc.ulp32(a[0][i]), (i, a[0][i], b[0][i])
    assert a[0][7] == b[0][7] == 0


def test_lambda_box_scales_the_box_gradient_only(lib, dev):
    c = br.case_by_name("small")
    for kind in br.KINDS:
        l8, g, dense, acc = run(lib, dev, c, br.KIND_ID[kind], lam=0.75)
        rep = br.judge(c, kind, l8, g, lambda_box=0.75)
        assert rep.ok, "\n".join(rep.failures)
        _check_acc(c, acc, l8, br.reference(c, kind, 0.75), lam=0.75)
        _check_against_ex(c, l8, g, dense, _ex_result(lib, dev, c))
    l8, g, _, _ = run(lib, dev, c, br.KIND_ID["giou"], lam=0.0)
    s5 = (c.N, c.A, 5 + c.C, c.fh, c.fw)
    assert (g.reshape(s5)[:, :, :4] == 0).all() and l8[1] > 0 and l8[0] == np.float32(np.float32(l8[5]) + np.float32(l8[6]))


def test_refusals(lib, dev):
    from yolo_fastest_amd import _lib
    c = br.case_by_name("e17")
    need = lr.need(lib, c, "box")
    n = ctypes.c_size_t()
    assert lib.yf_train_head_loss_box_workspace_bytes(c.N, c.fh, c.fw, 9, c.C, ctypes.byref(n)) == _lib.YF_E_INVALID
    assert lib.yf_train_head_loss_box_workspace_bytes(c.N, c.fh, c.fw, c.A, 0, ctypes.byref(n)) == _lib.YF_E_INVALID
    assert lib.yf_train_head_loss_box_workspace_bytes(c.N, c.fh, c.fw, c.A, c.C, None) == _lib.YF_E_INVALID
    x, t = torch.from_numpy(c.logits).to(dev), torch.from_numpy(c.targets).to(dev)
    work, losses = lr.Guarded(need + 8, dev), lr.Guarded(32, dev)
    anc9 = (ctypes.c_double * 18)(*([16.0, 30.0] * 9))

    def call(A=None, C=None, T=None, ptr=work.ptr, nbytes=need, anc=None, kind=3, lam=LAM):
        return lr.call(lib, "box", c, x, t, ptr, nbytes, losses.ptr, None, None, kind, lam, A=A, C=C, T=T, anchors=anc)
    for kind in (-1, 4, 255):
        assert call(kind=kind) == _lib.YF_E_INVALID and b"box_kind" in lib.yf_last_error_string()
    for lam in (-1.0, -1e-300, float("nan"), float("inf"), float("-inf")):
        assert call(lam=lam) == _lib.YF_E_INVALID and b"lambda_box" in lib.yf_last_error_string()
    assert call(lam=-1.0, kind=0) == _lib.YF_E_INVALID
    assert call(T=0) == _lib.YF_E_INVALID
    assert call(A=9, anc=anc9, nbytes=1 << 20) == _lib.YF_E_INVALID
    assert call(C=0) == _lib.YF_E_INVALID
    assert call(nbytes=need - 1) == _lib.YF_E_WORKSPACE
    assert call(nbytes=lr.need(lib, c, "ex")) == _lib.YF_E_WORKSPACE          # yf_train_head_loss_ex's size is two planes short
    assert call(ptr=work.ptr + 4) == _lib.YF_E_INVALID and b"aligned" in lib.yf_last_error_string()
    torch.cuda.synchronize(dev)
    assert (work.buf == 0xA5).all() and (losses.buf == 0xA5).all()          # a refused call launches nothing
    assert call() == 0 and call(lam=0.0) == 0
    torch.cuda.synchronize(dev)
    assert work.guards_untouched() and losses.guards_untouched()


def test_through_YOLOLossV3(lib, dev):
    """validation.YOLOLossV3(..., box_loss=kind)(pred, targets): the C entry's numbers as (loss, box, 0.0, 0.0, 0.0, conf, cls); the gradient
    scales through backward(); non-contiguous and float64 inputs; IndexError for what the reference cannot index; and without box_loss
    still yf_train_head_loss_ex bit for bit."""
    from yolo_fastest_amd import validation as val
    c = br.case_by_name("small")
    t = torch.from_numpy(c.targets).to(dev)
    for kind, lam in (("giou", LAM), ("diou", LAM), ("ciou", LAM), ("ciou", 0.75)):
        l8, g, _, _ = run(lib, dev, c, br.KIND_ID[kind], lam=lam)
        crit = val.YOLOLossV3(c.anchors, c.C, [c.H, c.W, 1], dev, box_loss=kind, lambda_box=lam)
        x = torch.from_numpy(c.logits).to(dev).requires_grad_(True)
        out = crit(x, t)
        assert len(out) == 7 and out[2:5] == (0.0, 0.0, 0.0)
        got = np.array([out[0].item()] + list(out[1:]) + [0.0], np.float32)
        assert br.judge(c, kind, got, lambda_box=lam).ok
        for i in range(7):
            assert abs(float(got[i]) - float(l8[i])) <= lc.ulp32(l8[i])
        (3.0 * out[0]).backward()
        assert torch.equal(x.grad.cpu(), 3.0 * torch.from_numpy(g))
    # (crit: ciou, 0.75) a non-contiguous view of the same values, and float64
    base = torch.from_numpy(np.ascontiguousarray(c.logits.transpose(0, 2, 3, 1))).to(dev).requires_grad_(True)
    xn = base.permute(0, 3, 1, 2)
    assert not xn.is_contiguous()
    out_n = crit(xn, t)
    out_n[0].backward()
    assert torch.equal(base.grad.permute(0, 3, 1, 2).cpu(), torch.from_numpy(g))
    x64 = torch.from_numpy(c.logits).double().to(dev).requires_grad_(True)
    out_d = crit(x64, t)
    out_d[0].backward()
    assert x64.grad.dtype == torch.float64 and torch.equal(x64.grad.float().cpu(), torch.from_numpy(g))
    for o in (out_n, out_d):
        assert br.judge(c, "ciou", np.array([o[0].item()] + list(o[1:]) + [0.0], np.float32), lambda_box=0.75).ok
    # the default: yf_train_head_loss_ex
    el8, eg, _, _ = _ex_result(lib, dev, c)
    x = torch.from_numpy(c.logits).to(dev).requires_grad_(True)
    out = val.YOLOLossV3(c.anchors, c.C, [c.H, c.W, 1], dev)(x, t)
    out[0].backward()
    assert torch.equal(x.grad.cpu(), torch.from_numpy(eg))
    assert all(abs(float(a) - float(b)) <= lc.ulp32(b) for a, b in zip([out[0].item()] + list(out[1:]), el8[:7]))
    assert lc.judge(c, np.array([out[0].item()] + list(out[1:]) + [0.0], np.float32)).ok
    # what the reference cannot index
    c = br.case_by_name("counted")
    crit = val.YOLOLossV3(c.anchors, c.C, [c.H, c.W, 1], dev, box_loss="giou")
    with pytest.raises(IndexError, match="^5 target"):
        crit(torch.from_numpy(c.logits).to(dev), torch.from_numpy(c.targets).to(dev))


def test_measured_worst_ratio_per_kind(lib, dev, capsys):
    """prints the MEASURED table: per box kind and judged quantity, over the judged cases, the worst distance / bound, the case, and the
    device's and the twin's distances"""
    lines, ok = [], True
    for kind in br.KINDS:
        worst = {}
        for c in CASES:
            if c.logit_set == "band":
                continue
            l8, g, dense, _ = _result(lib, dev, c, kind)
            for what, d, tw, bound in br.judge(c, kind, l8, g).rows:
                if not math.isnan(d) and bound > 0:
                    r = d / bound
                    if what not in worst or r > worst[what][0]:
                        worst[what] = (r, c.name, d, tw, "ulp floor" if bound > lc.ACCURACY_RATIO * tw else "3 x twin")
        for what, (r, name, d, tw, which) in worst.items():
            if what in ("loss total", "loss box", "grad box"):
                lines.append("  %-5s %-11s %.2f  %-13s device %.2e  twin %.2e  %s" % (kind, what, r, name, d, tw, which))
            ok = ok and r <= 1
    with capsys.disabled():
        print("\n[box loss: worst distance / bound per kind]\n" + "\n".join(lines))
    assert ok
