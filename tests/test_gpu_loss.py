"""The training loss of one head on the device -- loss_init_kernel, loss_targets_kernel, loss_cells_kernel<GRAD>, loss_final_kernel
(csrc/yf_loss_kernels.hip) behind yf_train_head_loss_workspace_bytes_ex / yf_train_head_loss_ex, called through ctypes -- against the
float64 model of oracle/loss_oracle.py::loss_model64, per term kind, on the case table of tests/loss_cases.py (its docstring states the
cases and the comparator; tests/test_cpu_loss_cases.py shows on the CPU that every case has its property, that the fp32 twin is inside
the table's condition and that the comparator rejects every planted defect).

Per case: the dense target planes are read back from the workspace behind its 16 doubles ([6 + C][E] float32, the layout
include/yolo_fastest_hip.h states) and compared bit for bit with get_target (tw, th: one ulp); losses[7] exactly; the seven losses and the
gradient per kind against max(3 x the twin's distance, the ulp floor).  The workspace is exactly the reported size; it, d_losses[8] and
d_grad_head each sit between two 4 KiB guards of 0xA5 bytes that must come back untouched; the gradient is pre-filled with a NaN pattern
and must come back fully written (tests/loss_run.py, the one runner of the three loss entries).

Two runs of one case give the same gradient bits (no atomic feeds it: loss_cells_kernel<true> reads the finished n_pos) but NOT
necessarily the same seven sums: those are double atomicAdds of one partial per workgroup, whose order differs from run to run; a
different order moves a double sum by a few 1e-16 relative, which can move the float32 result by one ulp at most.  So the sums are
asserted within one float32 ulp, the gradient bit-identical.

MEASURED (MI355X; per kind the worst case of the table: distance to the model / the bound it is held to, then the case, the device's
and the twin's distance and which side of the max() the bound is; test_measured_worst_ratio_per_kind prints it; no bound comes from it):
  loss total       0.58  edges        device 5.62e-07  twin 3.24e-07  3 x twin
  loss x           0.41  e17          device 1.54e-07  twin 1.24e-07  3 x twin
  loss y           0.43  e255         device 6.65e-08  twin 5.16e-08  3 x twin
  loss w           0.11  counted      device 1.67e-09  twin 1.92e-10  ulp floor
  loss h           0.16  skipped      device 9.42e-09  twin 9.42e-09  ulp floor
  loss conf        0.54  a8c20        device 2.58e-07  twin 1.39e-07  ulp floor
  loss cls         0.54  large        device 5.15e-07  twin 2.77e-07  ulp floor
  grad x           0.68  e17          device 2.02e-08  twin 6.57e-09  ulp floor
  grad y           0.56  edges        device 2.91e-10  twin 1.75e-10  3 x twin
  grad w           0.33  e255         device 1.96e-08  twin 1.96e-08  ulp floor
  grad h           0.30  n64          device 1.13e-09  twin 1.13e-09  ulp floor
  grad conf_pos    0.58  e15          device 8.69e-09  twin 3.99e-09  ulp floor
  grad conf_noobj  0.55  roundup      device 1.40e-10  twin 8.54e-11  3 x twin
  grad cls         0.58  cell_same_S  device 1.74e-08  twin 9.93e-09  3 x twin
  box_off, conf_ignored, cls_off: exactly zero in every case; tw / th values not identical to the host's: 0 in every case.
One run of a library whose yf_loss_kernels.hip was built with -ffp-contract=fast: the planes stay identical (this compiler packs the two
area products into one v_pk_mul_f32 and does not fuse the union), six cases fail on loss_final_kernel's total (_check_acc recomputes
d_losses from the 16 doubles exactly) and on e3_S's class gradient.
The whole file (46 tests) takes 3.6 s on one MI355X.
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
import loss_cases as lc  # noqa: E402
import loss_run as lr  # noqa: E402

CASES = lc.cases()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from yolo_fastest_amd import _lib
    return _lib.lib()


def run(lib, dev, c, grad=True, stream=None):
    return lr.run(lib, dev, c, "ex", grad=grad, stream=stream)


_results = {}


def _result(lib, dev, c):
    if c.name not in _results:
        _results[c.name] = run(lib, dev, c)
    return _results[c.name]


def _check_acc(c, acc, l8, ref):
    """the workspace's 16 doubles as the header states them: d_losses is loss_final_kernel's float32 arithmetic on exactly these"""
    F = np.float32
    E = float(c.N * c.A * c.fh * c.fw)
    assert acc[7] == ref["m64"]["n_pos"] and acc[8] == ref["counted"] and (acc[9:] == 0).all(), (c.name, acc)
    with np.errstate(invalid="ignore", divide="ignore"):
        lx, ly, lw, lh = (F(acc[i] / E) for i in range(4))
        lconf = F(F(acc[4] / E) + F(0.5) * F(acc[5] / E))
        lcls = F(acc[6] / (c.C * acc[7]))
        total = F(F(F(F(F(lx * F(2.5) + ly * F(2.5)) + lw * F(2.5)) + lh * F(2.5)) + lconf) + lcls)
    want = np.array([total, lx, ly, lw, lh, lconf, lcls, acc[8]], np.float32)
    assert np.array_equal(want, l8, equal_nan=True), (c.name, want, l8)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_case_against_the_float64_model(lib, dev, capsys, case):
    ref = lc.reference(case)
    l8, g, dense, acc = _result(lib, dev, case)
    rep = lc.judge(case, l8, g, dense, ref)
    with capsys.disabled():
        print("\n" + rep.table())
    _check_acc(case, acc, l8, ref)
    assert rep.ok, "\n".join(rep.failures)


def test_whole_table_without_the_gradient(lib, dev):
    """d_grad_head = NULL, the validation-time call: the same planes, counter and losses"""
    bad = []
    for c in CASES:
        l8, g, dense, acc = run(lib, dev, c, grad=False)
        rep = lc.judge(c, l8, None, dense)
        _check_acc(c, acc, l8, lc.reference(c))
        bad += rep.failures
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", ["e17", "n130", "thres_S", "nopos"])
def test_on_a_stream_of_its_own(lib, dev, name):
    c = lc.case_by_name(name)
    s = torch.cuda.Stream(dev)
    assert s.cuda_stream != torch.cuda.current_stream(dev).cuda_stream
    l8, g, dense, _ = run(lib, dev, c, stream=s)
    rep = lc.judge(c, l8, g, dense)
    assert rep.ok, "\n".join(rep.failures)
    assert np.array_equal(g.view(np.int32), _result(lib, dev, c)[1].view(np.int32))


@pytest.mark.parametrize("name", ["large", "n130", "small_S", "thres"])
def test_two_runs_give_the_same_gradient_bits_and_sums_within_one_ulp(lib, dev, name):
    """(see the module docstring: the gradient is fed by no atomic, the seven sums are double atomicAdds across workgroups)"""
    c = lc.case_by_name(name)
    assert c.N * c.A * c.fh * c.fw > 256                    # more than one workgroup adds to each sum
    a, b = run(lib, dev, c), run(lib, dev, c)
    assert np.array_equal(a[1].view(np.int32), b[1].view(np.int32))
    assert np.array_equal(a[2].view(np.int32), b[2].view(np.int32))
    for i in range(7):
        assert abs(float(a[0][i]) - float(b[0][i])) <= lc.ulp32(a[0][i]), (i, a[0][i], b[0][i])
    assert a[0][7] == b[0][7] == 0


def test_through_YOLOLossV3(lib, dev):
    """validation.YOLOLossV3(...)(pred, targets): the same numbers as the C entry; IndexError for what the reference cannot index; the
    gradient scales through backward(); non-contiguous and float64 inputs."""
    from yolo_fastest_amd import validation as val
    c = lc.case_by_name("small")
    l8, g, _, _ = _result(lib, dev, c)
    crit = val.YOLOLossV3(c.anchors, c.C, [c.H, c.W, 1], dev)
    t = torch.from_numpy(c.targets).to(dev)
    x = torch.from_numpy(c.logits).to(dev).requires_grad_(True)
    out = crit(x, t)
    rep = lc.judge(c, np.array([out[0].item()] + list(out[1:]) + [0.0], np.float32))
    assert rep.ok, rep.failures
    (3.0 * out[0]).backward()
    assert torch.equal(x.grad.cpu(), 3.0 * torch.from_numpy(g))
    # a non-contiguous view of the same values, and float64
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
        assert lc.judge(c, np.array([o[0].item()] + list(o[1:]) + [0.0], np.float32)).ok
    # what the reference cannot index: IndexError, each kind on its own and the message's count
    c = lc.case_by_name("counted")
    crit = val.YOLOLossV3(c.anchors, c.C, [c.H, c.W, 1], dev)
    x = torch.from_numpy(c.logits).to(dev)
    with pytest.raises(IndexError, match="^5 target"):
        crit(x, torch.from_numpy(c.targets).to(dev))
    for n, k in ((0, 0), (1, 0), (2, 0), (2, 1), (2, 2)):       # class C, class -1, column -1, column fw, row fh + 1
        one = np.zeros_like(c.targets)
        one[n, 0] = c.targets[n, k]
        with pytest.raises(IndexError, match="^1 target"):
            crit(x, torch.from_numpy(one).to(dev))
    ok = c.targets.copy()
    ok[0, 0] = 0; ok[1, 0, 4] = 2; ok[2, :3, 2] = 0             # the same batch with the five removed or mended
    assert math.isfinite(crit(x, torch.from_numpy(ok).to(dev))[0].item())


def test_refusals(lib, dev):
    from yolo_fastest_amd import _lib
    c = lc.case_by_name("e17")
    need = lr.need(lib, c, "ex")
    n = ctypes.c_size_t()
    assert lib.yf_train_head_loss_workspace_bytes_ex(c.N, c.fh, c.fw, 9, c.C, ctypes.byref(n)) == _lib.YF_E_INVALID
    assert lib.yf_train_head_loss_workspace_bytes_ex(c.N, c.fh, c.fw, c.A, 0, ctypes.byref(n)) == _lib.YF_E_INVALID
    x, t = torch.from_numpy(c.logits).to(dev), torch.from_numpy(c.targets).to(dev)
    work, losses = lr.Guarded(need + 8, dev), lr.Guarded(32, dev)
    anc9 = (ctypes.c_double * 18)(*([16.0, 30.0] * 9))

    def call(A=None, C=None, T=None, ptr=work.ptr, nbytes=need, anc=None):
        return lr.call(lib, "ex", c, x, t, ptr, nbytes, losses.ptr, None, None, A=A, C=C, T=T, anchors=anc)
    assert call(T=0) == _lib.YF_E_INVALID
    assert call(A=9, anc=anc9, nbytes=1 << 20) == _lib.YF_E_INVALID
    assert call(C=0) == _lib.YF_E_INVALID
    assert call(nbytes=need - 1) == _lib.YF_E_WORKSPACE
    assert call(ptr=work.ptr + 4) == _lib.YF_E_INVALID and b"aligned" in lib.yf_last_error_string()
    torch.cuda.synchronize(dev)
    assert (work.buf == 0xA5).all() and (losses.buf == 0xA5).all()          # a refused call launches nothing
    assert call() == 0
    torch.cuda.synchronize(dev)
    assert work.guards_untouched() and losses.guards_untouched()


def test_measured_worst_ratio_per_kind(lib, dev, capsys):
    """prints the MEASURED table: per kind, over the judged cases, the worst distance / bound, the case, and device and twin distances"""
    worst = {}
    for c in CASES:
        if c.logit_set == "band":
            continue
        l8, g, dense, _ = _result(lib, dev, c)
        rep = lc.judge(c, l8, g, dense)
        for what, d, tw, bound in rep.rows:
            if not math.isnan(d) and bound > 0:
                r = d / bound
                if what not in worst or r > worst[what][0]:
                    worst[what] = (r, c.name, d, tw, "ulp floor" if bound > lc.ACCURACY_RATIO * tw else "3 x twin")
    with capsys.disabled():
        print("\n[loss: worst distance / bound per kind]")
        for what, (r, name, d, tw, which) in worst.items():
            print("  %-16s %.2f  (%s: device %.2e, twin %.2e, bound = %s)" % (what, r, name, d, tw, which))
    assert all(v[0] <= 1 for v in worst.values())
