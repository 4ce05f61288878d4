"""training.ModelEMA, what needs no GPU: the arithmetic the kernels must compute (tests/ema_cases.py: ema_model) against yolov5's loop on
torch CPU float32 tensors, bit for bit -- it documents the kernels' contract and passes without them, the proof is tests/test_gpu_ema.py --,
the ramp, the argument checks of yf_train_ema_multi_pinned and yf_train_opt_ema_multi_pinned, which return before the GPU is touched, the
binding of the two symbols, and the ValueErrors of the constructor, update() and load_state_dict()."""
import ctypes
import inspect
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ema_cases as ec  # noqa: E402
import yolo_fastest_amd as yf  # noqa: E402
from yolo_fastest_amd import _lib, training  # noqa: E402


# ---- 1. the three-rounding model of yolov5's update ----
def test_the_fma_case_tells_a_fused_multiply_add_apart():
    name, e, p = ec.cases()[ec.FMA_CASE]
    assert name.startswith("fma") and len(e) == 256
    for i, u in enumerate(ec.UPDATES):
        d = ec.ramp(u)
        a, b = ec.fused_models(e, p, d)
        want = ec.ema_model(e, p, d)
        da, db = ec.bits(a) != ec.bits(want), ec.bits(b) != ec.bits(want)
        print("updates %7d: fma(e, d, (1-d) p) differs in %3d of 256, fma(1-d, p, e d) in %3d" % (u, int(da.sum()), int(db.sum())))
        own = slice(64 * i, 64 * i + 64)               # the 64 elements picked for this d: each tells both forms apart
        assert da[own].all() and db[own].all(), u


def test_the_model_is_yolov5s_loop_bit_for_bit():
    """yolov5's `v *= d; v += (1 - d) * msd[k].detach()` on float32 CPU tensors with d a Python double, carried through every d in turn."""
    cases = ec.cases()
    mine = [e.copy() for _, e, _ in cases]
    theirs = [torch.from_numpy(e.copy()) for _, e, _ in cases]
    msd = [torch.from_numpy(p.copy()) for _, _, p in cases]
    seen_nan = seen_sub = 0
    for d in ec.d_values():
        for i, (name, _, p) in enumerate(cases):
            v = theirs[i]
            v *= d
            v += (1 - d) * msd[i].detach()
            mine[i] = ec.ema_model(mine[i], p, d)
            assert ec.same_bits_or_nan(v.numpy(), mine[i]), (d, name)
            seen_nan += int(np.isnan(mine[i]).sum())
            seen_sub += int(((np.abs(mine[i]) < np.finfo(np.float32).tiny) & (mine[i] != 0)).sum())
    assert seen_nan > 0 and seen_sub > 0               # the cases reach both
    zeros = ec.ema_model(cases[3][1][:4], cases[3][2][:4], ec.ramp(1))
    assert np.signbit(zeros).tolist() == [False, False, False, True]          # only -0 d + (1 - d) -0 keeps the sign


def test_decay_is_the_closed_form():
    m = ec.toy_module([np.zeros(3, np.float32)], torch)
    ema = training.ModelEMA(m)
    assert ema.updates == 0 and ema.decay(0) == 0.0
    for x in (1, 2, 17, 2000, 10 ** 6):
        assert ema.decay(x) == 0.9999 * (1 - math.exp(-x / 2000)) == ec.ramp(x)
    other = training.ModelEMA(m, decay=0.99, tau=50, updates=12)
    assert other.updates == 12 and other.decay(7) == 0.99 * (1 - math.exp(-7 / 50))
    assert abs(ec.ramp(1) - 5e-4) < 1e-6 and 0.9998 < ec.ramp(10 ** 6) <= 0.9999


# ---- 2. the C entries ----
def test_both_entries_are_exported_and_declared():
    lib = _lib.lib()
    for name in ("yf_train_ema_multi_pinned", "yf_train_opt_ema_multi_pinned"):
        assert name in _lib.EXPORTS
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(_lib._SIGS[name][1])
    assert len(_lib._SIGS["yf_train_ema_multi_pinned"][1]) == 11
    assert len(_lib._SIGS["yf_train_opt_ema_multi_pinned"][1]) == len(_lib._SIGS["yf_train_opt_multi_pinned"][1]) + 6
    assert (_lib.YF_OPT_TABLE_ENTRY_BYTES, _lib.YF_OPT_EMA_TABLE_ENTRY_BYTES, _lib.YF_EMA_TABLE_ENTRY_BYTES) == (56, 64, 32)
    header = open(os.path.join(os.path.dirname(HERE), "include", "yolo_fastest_hip.h")).read()
    for text in ("#define YF_OPT_TABLE_ENTRY_BYTES 56", "#define YF_OPT_EMA_TABLE_ENTRY_BYTES 64", "#define YF_EMA_TABLE_ENTRY_BYTES 32",
                 "int yf_train_ema_multi_pinned(", "int yf_train_opt_ema_multi_pinned("):
        assert text in header, text


def _arr(v):
    return (ctypes.c_void_p * len(v))(*v)


def test_ema_entry_refuses_bad_arguments_without_a_gpu():
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(512)
    a = ctypes.addressof(buf)                          # never read as device memory: every call below is refused before a launch
    b = a + 256
    n = 2
    good = dict(n=n, src=_arr([a, a]), ema=_arr([b, b]), sizes=[4, 4], d=0.5, table=a, table_bytes=_lib.YF_EMA_TABLE_ENTRY_BYTES * n)

    def call(**change):
        g = dict(good, **change)
        sizes = (ctypes.c_long * n)(*g["sizes"]) if g["sizes"] is not None else None
        return lib.yf_train_ema_multi_pinned(0, g["n"], g["src"], g["ema"], sizes, g["d"], g["table"], g["table_bytes"], None, 1, None)
    bad = [dict(src=None), dict(ema=None), dict(sizes=None), dict(table=None), dict(n=0), dict(n=-1),
           dict(table_bytes=_lib.YF_EMA_TABLE_ENTRY_BYTES * n - 1), dict(src=_arr([a, None])), dict(ema=_arr([None, b])),
           dict(sizes=[4, 0]), dict(sizes=[-1, 4]), dict(ema=_arr([b, a])),                                   # an EMA pointer equal to its source
           dict(d=-1e-9), dict(d=1.0 + 1e-9), dict(d=float("nan")), dict(d=float("inf")), dict(d=-float("inf"))]
    for change in bad:
        assert call(**change) == _lib.YF_E_INVALID, change
        assert b"yf_train_ema_multi" in lib.yf_last_error_string()
    with pytest.raises(_lib.YFError, match=r"\[0, 1\]"):
        _lib.check(call(d=2.0))


def test_opt_ema_entry_refuses_bad_arguments_without_a_gpu():
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(512)
    a = ctypes.addressof(buf)
    b = a + 256
    n = nx = 2
    eb = _lib.YF_OPT_EMA_TABLE_ENTRY_BYTES

    def group(**kw):
        g = dict(lr=0.01, weight_decay=5e-4, momentum=0.9, dampening=0.0, beta1=0.9, beta2=0.999, eps=1e-8, nesterov=1, step=1, maximize=0)
        g.update(kw)
        return g
    good = dict(kind=_lib.YF_OPT_SGD, n=n, p=_arr([a, a]), g=_arr([a, a]), s1=_arr([a, a]), s2=_arr([a, a]), sizes=[4, 4], gof=[0, 1],
                first=[0, 0], groups=[group(), group()], ema=_arr([b, b]), nx=nx, xs=_arr([a, a]), xe=_arr([b, b]), xn=[4, 4], d=0.5, table=a,
                table_bytes=eb * (n + nx))

    def call(**change):
        g = dict(good, **change)
        ng = len(g["groups"])
        og = (_lib.OptGroup * max(ng, 1))()
        for o, q in zip(og, g["groups"]):
            for k, v in q.items():
                setattr(o, k, v)
        sizes = (ctypes.c_long * n)(*g["sizes"]) if g["sizes"] is not None else None
        gof = (ctypes.c_int * n)(*g["gof"]) if g["gof"] is not None else None
        first = (ctypes.c_int * n)(*g["first"]) if g["first"] is not None else None
        xn = (ctypes.c_long * len(g["xn"]))(*g["xn"]) if g["xn"] is not None else None
        return lib.yf_train_opt_ema_multi_pinned(0, g["kind"], g["n"], g["p"], g["g"], g["s1"], g["s2"], sizes, gof, first, ng,
                                                 og if g.get("og", True) else None, g["ema"], g["nx"], g["xs"], g["xe"], xn, g["d"], g["table"],
                                                 g["table_bytes"], None, 1, None)
    bad = [  # what the new arguments add
           dict(ema=None), dict(ema=_arr([b, None])), dict(ema=_arr([a, b])), dict(nx=-1), dict(xs=None), dict(xe=None), dict(xn=None),
           dict(xs=_arr([a, None])), dict(xe=_arr([None, b])), dict(xe=_arr([b, a])), dict(xn=[4, 0]), dict(xn=[-3, 4]),
           dict(d=-1e-9), dict(d=1.0 + 1e-9), dict(d=float("nan")), dict(d=float("inf")),
           dict(table_bytes=eb * (n + nx) - 1), dict(table_bytes=_lib.YF_OPT_TABLE_ENTRY_BYTES * (n + nx)), dict(nx=0, table_bytes=eb * n - 1),
           # everything yf_train_opt_multi_pinned refuses (tests/test_cpu_optim.py)
           dict(p=None), dict(g=None), dict(sizes=None), dict(gof=None), dict(og=False), dict(table=None), dict(n=0), dict(n=-1),
           dict(kind=2), dict(kind=-1), dict(p=_arr([a, None])), dict(g=_arr([None, a])), dict(s1=_arr([a, None])), dict(s1=None),
           dict(sizes=[4, 0]), dict(sizes=[-1, 4]), dict(gof=[0, 2]), dict(gof=[-1, 0]),
           dict(groups=[]), dict(groups=[group()] * 9, gof=[0, 8]),
           dict(groups=[group(), group(dampening=0.1)]), dict(groups=[group(maximize=1), group()]),
           dict(groups=[group(), group(momentum=0.0)]), dict(groups=[group(momentum=-0.1), group()]),
           dict(kind=_lib.YF_OPT_ADAM, groups=[group(), group(step=0)]), dict(kind=_lib.YF_OPT_ADAM, s2=None),
           dict(kind=_lib.YF_OPT_ADAM, s2=_arr([a, None])), dict(kind=_lib.YF_OPT_ADAM, groups=[group(maximize=1), group()])]
    for change in bad:
        assert call(**change) == _lib.YF_E_INVALID, change
        assert b"yf_train_opt_ema_multi" in lib.yf_last_error_string()
    with pytest.raises(_lib.YFError, match="dampening"):
        _lib.check(call(groups=[group(dampening=0.5), group()]))


# ---- 3. ModelEMA's own refusals and its state-dict ----
@pytest.fixture(scope="module")
def net():
    return yf.YoloFastest(yf.io_params_for(256))


def test_ema_is_an_eval_copy_built_from_io_params(net):
    net.train()
    torch.manual_seed(5)
    want = torch.rand(3)
    torch.manual_seed(5)
    ema = training.ModelEMA(net)
    assert torch.equal(torch.rand(3), want)            # building the copy leaves the caller's random stream alone (train()'s shuffle)
    assert type(ema.ema) is type(net) and ema.ema is not net and not ema.ema.training and net.training
    assert (ema.ema.num_cls, ema.ema.input_channel, ema.ema.num_anchors) == (net.num_cls, net.input_channel, net.num_anchors)
    assert all(not p.requires_grad for p in ema.ema.parameters()) and all(p.requires_grad for p in net.parameters())
    own, theirs = ema.ema.state_dict(), net.state_dict()
    assert list(own) == list(theirs) and len(own) == 508
    assert all(torch.equal(own[k], theirs[k]) and own[k].data_ptr() != theirs[k].data_ptr() for k in own)
    assert sum(v.is_floating_point() for v in own.values()) == 424 == len(ema._slots)
    assert [k for k, _, _ in ema._slots] == [k for k, v in own.items() if v.is_floating_point()]
    sig = inspect.signature(training.ModelEMA.__init__).parameters
    assert [sig[k].default for k in ("decay", "tau", "updates")] == [0.9999, 2000, 0]
    with pytest.raises(RuntimeError, match="no CPU path"):
        ema.update(net)
    assert inspect.signature(training.train).parameters["ema"].default is False
    assert inspect.signature(training.train_step).parameters["ema"].default is None
    assert inspect.signature(training.SGD.step).parameters["ema"].default is None


def test_constructor_and_update_refuse_a_model_of_other_keys_or_shapes(net):
    odd = yf.YoloFastest(yf.io_params_for(256))
    odd.conv0[1].register_buffer("extra_stat", torch.zeros(8))                 # a floating entry the rebuilt network does not have
    with pytest.raises(ValueError, match="keys"):
        training.ModelEMA(odd)
    wide = yf.YoloFastest(yf.io_params_for(256))
    wide.head_5.bias = torch.nn.Parameter(torch.zeros(wide.head_5.bias.numel() + 1))
    with pytest.raises(ValueError, match="head_5.bias"):
        training.ModelEMA(wide)
    ema = training.ModelEMA(net)
    for other in (odd, wide):
        with pytest.raises(ValueError):
            ema.update(other)
    assert ema.updates == 0                            # refused before anything moved
    io5 = yf.io_params_for(256)
    io5["num_cls"] = 5
    with pytest.raises(ValueError, match="head_"):
        ema.update(yf.YoloFastest(io5))
    for kw in (dict(decay=1.5), dict(decay=-0.1), dict(tau=0), dict(updates=-1)):
        with pytest.raises(ValueError, match="ModelEMA"):
            training.ModelEMA(net, **kw)


def test_state_dict_round_trip_and_its_refusals(net):
    ema = training.ModelEMA(net, updates=41)
    sd = ema.state_dict()
    assert len(sd) == 509 and sd["updates"] == 41 and [k for k in sd if k != "updates"] == list(net.state_dict())
    changed = {k: (v + 1 if k != "updates" else 77) for k, v in sd.items()}
    fresh = training.ModelEMA(net)
    fresh.ema._blob = object()                         # (stands for packed weights: a load must drop them)
    fresh.load_state_dict(changed)
    assert fresh.updates == 77 and fresh.ema._blob is None
    got = fresh.ema.state_dict()
    assert all(torch.equal(got[k], changed[k]) for k in got)
    assert int(got["conv0.1.num_batches_tracked"]) == int(sd["conv0.1.num_batches_tracked"]) + 1
    before = fresh.state_dict()
    no_updates = {k: v for k, v in changed.items() if k != "updates"}
    missing = {k: v for k, v in changed.items() if k != "conv0.0.weight"}
    extra = dict(changed, bogus=torch.zeros(1))
    shape = dict(changed)
    shape["head_4.bias"] = torch.zeros(3)
    for bad, what in ((no_updates, "updates"), (missing, "conv0.0.weight"), (extra, "bogus"), (shape, "head_4.bias")):
        with pytest.raises(ValueError, match=what):
            fresh.load_state_dict(bad)
    after = fresh.state_dict()
    assert after["updates"] == 77 and all(torch.equal(after[k], before[k]) for k in got)      # a refused load changes nothing
