"""training.SGD / training.Adam / train()'s opt-in train_params keys, what needs no GPU: the SGD arithmetic the kernel must compute
(tests/optim_cases.py: sgd_model) against torch.optim.SGD on the CPU, bit for bit -- it documents the kernel's contract and passes without
the kernel, the proof is tests/test_gpu_optim.py --, the constructors' refusals, the argument checks of yf_train_opt_multi_pinned, which
return before the GPU is touched, and train()'s refusals, which come before a device is needed."""
import copy
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import optim_cases as oc  # noqa: E402
import yolo_fastest_amd as yf  # noqa: E402
from yolo_fastest_amd import _lib, training  # noqa: E402


# ---- 1. the four-line model of torch.optim.SGD ----
def test_fma32_rounds_once():
    f = np.float32
    a, b = f(1 + 2.0 ** -12), f(1 + 2.0 ** -12)                       # a b = 1 + 2^-11 + 2^-24: exact only in the fused form
    assert f(a * b) == f(1 + 2.0 ** -11)
    assert oc.fma32(a, b, f(-(1 + 2.0 ** -11)))[()] == f(2.0 ** -24)
    # a sum that rounding twice gets wrong: c + 64 - 2^-40 lies just below the midpoint of c and the next float32 (c has an odd last
    # bit, its ulp is 128); float64 cannot hold the 2^-40, lands on the midpoint, and the tie then goes up to the even neighbour
    a, b, c = f(8 + 2.0 ** -20), f(8 - 2.0 ** -20), f(2.0 ** 30 + 128)
    assert np.float64(a) * np.float64(b) == 64 - 2.0 ** -40
    assert f(np.float64(a) * np.float64(b) + np.float64(c)) == f(2.0 ** 30 + 256)
    assert oc.fma32(a, b, c)[()] == c
    assert oc.fma32(a, -b, -c)[()] == -c
    assert np.signbit(oc.fma32(f(5e-4), f(-0.0), f(-0.0))[()]) and not np.signbit(oc.fma32(f(0.0), f(1.0), f(-0.0))[()])


@pytest.mark.parametrize("which", ["one", "three"])
@pytest.mark.parametrize("cfg", oc.CONFIGS)
def test_the_model_is_torchs_sgd_bit_for_bit(cfg, which):
    mom, nesterov, wd = cfg
    groups = oc.layout(which, wd)
    ref = [torch.nn.Parameter(torch.from_numpy(a.copy())) for a in oc.parameters(3)]
    opt = torch.optim.SGD([dict(params=[ref[i] for i in idx], lr=lr, weight_decay=w) for idx, lr, w in groups], lr=0.01, momentum=mom,
                          nesterov=nesterov)
    mine = [a.copy() for a in oc.parameters(3)]
    bufs = [None] * len(mine)
    lrs = [lr for _, lr, _ in groups]
    for it in range(oc.STEPS):
        gs = oc.gradients(3, it)
        if it == 2:
            lrs = [lr * oc.LR_EDIT for lr in lrs]
            for grp, lr in zip(opt.param_groups, lrs):
                grp["lr"] = lr
        for p, g in zip(ref, gs):
            p.grad = None if g is None else torch.from_numpy(g.copy())
        opt.step()
        for (idx, _, w), lr in zip(groups, lrs):
            for i in idx:
                if gs[i] is not None:
                    mine[i], bufs[i] = oc.sgd_model(mine[i], gs[i], bufs[i], lr, mom, nesterov, w)
        for i, p in enumerate(ref):
            assert np.array_equal(oc.bits(mine[i]), oc.bits(p.detach().numpy())), (it, oc.SIZES[i])
            buf = opt.state[p].get("momentum_buffer") if p in opt.state else None
            assert (buf is None) == (bufs[i] is None)
            if buf is not None:
                assert np.array_equal(oc.bits(bufs[i]), oc.bits(buf.numpy())), (it, oc.SIZES[i])
                assert it > 0 or np.signbit(bufs[i][0])            # g = -0.0, p = -0.0: the first step's buffer keeps the sign


# ---- 2. constructors ----
def test_constructors_refuse_what_is_not_implemented():
    p = [torch.nn.Parameter(torch.zeros(3))]
    with pytest.raises(ValueError, match="dampening"):
        training.SGD(p, lr=0.1, momentum=0.9, dampening=0.1)
    with pytest.raises(ValueError, match="Nesterov"):
        training.SGD(p, lr=0.1, nesterov=True)
    with pytest.raises(ValueError, match="Nesterov"):
        torch.optim.SGD(p, lr=0.1, nesterov=True)                  # torch refuses the same
    with pytest.raises(ValueError):
        training.SGD(p, lr=0.1, momentum=-0.5)
    o = training.SGD(p, lr=0.1, momentum=0.9, weight_decay=1e-3, nesterov=True)
    assert isinstance(o, torch.optim.Optimizer)
    assert {k: o.param_groups[0][k] for k in ("lr", "momentum", "dampening", "weight_decay", "nesterov")} == \
        dict(lr=0.1, momentum=0.9, dampening=0, weight_decay=1e-3, nesterov=True)
    a = training.Adam([dict(params=p), dict(params=[torch.nn.Parameter(torch.zeros(2))], weight_decay=5e-4)], lr=0.01)
    assert [g["weight_decay"] for g in a.param_groups] == [0, 5e-4] and a.param_groups[0]["betas"] == (0.9, 0.999)
    p[0].grad = torch.ones(3)
    for opt in (o, a):
        with pytest.raises(RuntimeError, match="no CPU path"):
            opt.step()
    nine = training.SGD([dict(params=[torch.nn.Parameter(torch.zeros(1))]) for _ in range(9)], lr=0.1)
    with pytest.raises(ValueError, match="param groups"):
        nine.step()


def test_param_groups_are_yolov5s_three():
    m = yf.YoloFastest(yf.io_params_for(256))
    g = training.param_groups(m, 5e-4)
    assert [sorted(d) for d in g] == [["params"], ["params", "weight_decay"], ["params"]] and g[1]["weight_decay"] == 5e-4
    bn = [mod.weight for _, mod in m.named_modules() if isinstance(mod, torch.nn.BatchNorm2d)]
    w = [mod.weight for _, mod in m.named_modules() if isinstance(mod, (torch.nn.Conv2d, torch.nn.ConvTranspose2d))]
    b = [mod.bias for _, mod in m.named_modules() if getattr(mod, "bias", None) is not None]
    for got, want in zip(g, (bn, w, b)):
        assert len(got["params"]) == len(want) and all(x is y for x, y in zip(got["params"], want))
    ids = [id(p) for d in g for p in d["params"]]
    assert len(ids) == len(set(ids)) and set(ids) == {id(p) for p in m.parameters()}
    odd = torch.nn.Sequential(torch.nn.PReLU(), torch.nn.Bilinear(2, 2, 2))
    odd[1].extra = torch.nn.Parameter(torch.zeros(1))              # a parameter that is neither a .weight nor a .bias
    with pytest.raises(ValueError, match="param_groups"):
        training.param_groups(odd, 0.0)


# ---- 3. the C entry refuses bad arguments before the GPU is touched ----
def test_opt_entry_refuses_bad_arguments_without_a_gpu():
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(256)
    ptr = ctypes.addressof(buf)                      # never read as device memory: every call below is refused before a launch
    n = 2

    def arr(v):
        return (ctypes.c_void_p * n)(*v)

    def group(**kw):
        g = dict(lr=0.01, weight_decay=5e-4, momentum=0.9, dampening=0.0, beta1=0.9, beta2=0.999, eps=1e-8, nesterov=1, step=1, maximize=0)
        g.update(kw)
        return g
    good = dict(kind=_lib.YF_OPT_SGD, n=n, p=arr([ptr, ptr]), g=arr([ptr, ptr]), s1=arr([ptr, ptr]), s2=arr([ptr, ptr]), sizes=[4, 4], gof=[0, 1],
                first=[0, 0], groups=[group(), group()], table=ptr, table_bytes=_lib.YF_OPT_TABLE_ENTRY_BYTES * n)

    def call(**change):
        a = dict(good, **change)
        ng = len(a["groups"])
        og = (_lib.OptGroup * max(ng, 1))()
        for o, g in zip(og, a["groups"]):
            for k, v in g.items():
                setattr(o, k, v)
        sizes = (ctypes.c_long * n)(*a["sizes"]) if a["sizes"] is not None else None
        gof = (ctypes.c_int * n)(*a["gof"]) if a["gof"] is not None else None
        first = (ctypes.c_int * n)(*a["first"]) if a["first"] is not None else None
        return lib.yf_train_opt_multi_pinned(0, a["kind"], a["n"], a["p"], a["g"], a["s1"], a["s2"], sizes, gof, first, ng,
                                             og if a.get("og", True) else None, a["table"], a["table_bytes"], None, 1, None)
    bad = [dict(p=None), dict(g=None), dict(sizes=None), dict(gof=None), dict(og=False), dict(table=None), dict(n=0), dict(n=-1),
           dict(table_bytes=_lib.YF_OPT_TABLE_ENTRY_BYTES * n - 1), dict(kind=2), dict(kind=-1),
           dict(p=arr([ptr, None])), dict(g=arr([None, ptr])), dict(s1=arr([ptr, None])), dict(s1=None),          # momentum needs its buffer
           dict(sizes=[4, 0]), dict(sizes=[-1, 4]), dict(gof=[0, 2]), dict(gof=[-1, 0]),
           dict(groups=[]), dict(groups=[group()] * 9, gof=[0, 8]),
           dict(groups=[group(), group(dampening=0.1)]), dict(groups=[group(maximize=1), group()]),
           dict(groups=[group(), group(momentum=0.0)]),                                                           # nesterov without momentum
           dict(groups=[group(momentum=-0.1), group()]),
           dict(kind=_lib.YF_OPT_ADAM, groups=[group(), group(step=0)]), dict(kind=_lib.YF_OPT_ADAM, s2=None),
           dict(kind=_lib.YF_OPT_ADAM, s2=arr([ptr, None])), dict(kind=_lib.YF_OPT_ADAM, groups=[group(maximize=1), group()])]
    for change in bad:
        assert call(**change) == _lib.YF_E_INVALID, change
        assert b"yf_train_opt_multi" in lib.yf_last_error_string()
    with pytest.raises(_lib.YFError, match="dampening"):
        _lib.check(call(groups=[group(dampening=0.5), group()]))


# ---- 4. train() refuses before a device is needed ----
def test_train_refuses_an_unknown_optimizer_and_a_branch_weight_of_the_wrong_length(tmp_path):
    params = copy.deepcopy(yf.config_params)
    params["io_params"]["save_path"] = str(tmp_path / "models")
    items = [object()]                                             # never read
    with pytest.raises(ValueError, match="lamb"):
        training.train(params, None, train_dataset=items, optimizer="lamb")
    params["train_params"]["branch_weight"] = [1.0, 1.0, 1.0]
    with pytest.raises(ValueError, match="branch_weight"):
        training.train(params, None, train_dataset=items, branch_weight=True)
    assert not os.path.exists(params["io_params"]["save_path"])     # refused before anything was made
    import inspect
    sig = inspect.signature(training.train).parameters
    assert sig["optimizer"].default is None and sig["branch_weight"].default is False
    assert inspect.signature(training.train_step).parameters["branch_weight"].default is None
