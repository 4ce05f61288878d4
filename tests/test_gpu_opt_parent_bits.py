"""Adam through every entry that runs it (csrc/yf_train_opt_kernels.h: tadam_update behind yf_train_adam_step, yf_train_adam_multi,
yf_train_adam_multi_pinned, yf_train_opt_multi_pinned and yf_train_opt_ema_multi_pinned) against the bits of a recorded parent commit.

SGD and the EMA are held bit for bit to numpy models (tests/optim_cases.py, tests/ema_cases.py); Adam is held to torch only within 2e-7,
and its entries to each other.  tests/golden/opt_parent_bits.npz is the anchor from outside the code under test: what the commit named
in its `parent` entry leaves on an MI355X, as uint32 bits, after optim_cases.STEPS steps on optim_cases.parameters / gradients (seed 41)
at optim_cases.SIZES -- one element, an odd size, one short of / exactly / one past a 256-thread workgroup, several workgroups: the
smallest shapes at which the entry lookup and the tail guard can go wrong -- with every lr multiplied by LR_EDIT before step 3.

  adam_step          yf_train_adam_step, tensor by tensor                        p, m, v
  adam_multi         yf_train_adam_multi (no pinned copy)                        p, m, v           == adam_step
  adam_multi_pinned  yf_train_adam_multi_pinned, upload 1 then 0                 p, m, v           == adam_step
  adam_one           training.Adam, one group, weight_decay 0                    p, exp_avg, exp_avg_sq
  adam_three         training.Adam, optim_cases.layout("three", 5e-4)            p, exp_avg, exp_avg_sq
  adam_three_ema     the same through step(ema=) on ema_cases.toy_module         p, exp_avg, exp_avg_sq, ema   (p and moments == adam_three)

The legacy entries take every tensor in every step (the late tensor's missing first gradient is zeros); through training.Adam the late
tensor (index LATE) has no gradient in the first step, so from the second step on the step counts are mixed: one launch per count, and
with `ema` the average as a launch of its own.  Every stored array is the six tensors' bits one behind the other.

`python tests/test_gpu_opt_parent_bits.py --write <commit>` on a checkout of that commit (built) rewrites the fixture; the equalities
of the last column are asserted there too, so a parent that does not satisfy them cannot be recorded."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import ema_cases as ec  # noqa: E402
import optim_cases as oc  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "opt_parent_bits.npz")
SEED = 41
LR, BETAS, EPS = 0.001, (0.9, 0.999), 1e-08                    # the legacy entries and adam_one
BETAS3 = (0.937, 0.999)                                        # adam_three: the layout's own lr per group
CASES = ("adam_step", "adam_multi", "adam_multi_pinned", "adam_one", "adam_three", "adam_three_ema")
EQUAL = [("adam_multi", "adam_step", ("p", "m", "v")), ("adam_multi_pinned", "adam_step", ("p", "m", "v")),
         ("adam_three_ema", "adam_three", ("p", "m", "v"))]


def _bits(tensors):
    return np.concatenate([oc.bits(t.detach().cpu().numpy()) for t in tensors])


def _legacy(lib, check, dev, how):
    """STEPS steps through one of the yf_train_adam_* entries, called directly -> {p, m, v}"""
    n = len(oc.SIZES)
    p = [torch.from_numpy(a.copy()).to(dev) for a in oc.parameters(SEED)]
    m, v, g = [[torch.zeros_like(t) for t in p] for _ in range(3)]     # the gradients stay where they are: the table is uploaded once

    def arr(ts):
        return (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
    pa, ga, ma, va, sizes = arr(p), arr(g), arr(m), arr(v), (ctypes.c_long * n)(*oc.SIZES)
    table = torch.empty(48 * n, dtype=torch.uint8, device=dev)
    pinned = torch.empty(48 * n, dtype=torch.uint8).pin_memory()
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for it in range(oc.STEPS):
        for t, a in zip(g, oc.gradients(SEED, it)):
            t.copy_(torch.from_numpy(a if a is not None else np.zeros(t.numel(), np.float32)))
        lr = LR * oc.LR_EDIT if it >= 2 else LR
        if how == "adam_step":
            for i in range(n):
                check(lib.yf_train_adam_step(dev.index, p[i].data_ptr(), g[i].data_ptr(), m[i].data_ptr(), v[i].data_ptr(), oc.SIZES[i], lr,
                                             BETAS[0], BETAS[1], EPS, it + 1, stream))
        elif how == "adam_multi":
            check(lib.yf_train_adam_multi(dev.index, n, pa, ga, ma, va, sizes, lr, BETAS[0], BETAS[1], EPS, it + 1, table.data_ptr(),
                                          table.numel(), stream))
        else:
            check(lib.yf_train_adam_multi_pinned(dev.index, n, pa, ga, ma, va, sizes, lr, BETAS[0], BETAS[1], EPS, it + 1, table.data_ptr(),
                                                 table.numel(), pinned.data_ptr(), int(it == 0), stream))
    torch.cuda.synchronize()
    return dict(p=_bits(p), m=_bits(m), v=_bits(v))


def _through_training(training, dev, how):
    """STEPS steps of training.Adam -> {p, m, v (exp_avg, exp_avg_sq)[, ema]}"""
    if how == "adam_three_ema":
        mod = ec.toy_module(oc.parameters(SEED), torch).to(dev)
        ps = [getattr(mod, "p%d" % i) for i in range(len(oc.SIZES))]
        ema = training.ModelEMA(mod, updates=1999)                 # d ~ 0.63: both products of the average count
    else:
        ps = [torch.nn.Parameter(torch.from_numpy(a.copy()).to(dev)) for a in oc.parameters(SEED)]
        ema = None
    if how == "adam_one":
        opt = training.Adam(ps, lr=LR, betas=BETAS, eps=EPS)
    else:
        opt = training.Adam([dict(params=[ps[i] for i in idx], lr=lr, weight_decay=w) for idx, lr, w in oc.layout("three", 5e-4)], lr=LR,
                            betas=BETAS3, eps=EPS)
    for it in range(oc.STEPS):
        if it == 2:
            for grp in opt.param_groups:
                grp["lr"] = grp["lr"] * oc.LR_EDIT
        for q, a in zip(ps, oc.gradients(SEED, it)):
            q.grad = None if a is None else torch.from_numpy(a).to(dev)
        if ema is None:
            opt.step()
        else:
            opt.step(ema=ema)
    torch.cuda.synchronize()
    assert sorted({opt.state[q]["step"] for q in ps}) == [oc.STEPS - 1, oc.STEPS]
    out = dict(p=_bits(ps), m=_bits([opt.state[q]["exp_avg"] for q in ps]), v=_bits([opt.state[q]["exp_avg_sq"] for q in ps]))
    if ema is not None:
        assert ema.updates == 1999 + oc.STEPS
        out["ema"] = _bits([getattr(ema.ema, "p%d" % i) for i in range(len(ps))] + [ema.ema.stat])
    return out


def _runs():
    from yolo_fastest_amd import _lib, training
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    out = {how: _legacy(_lib.lib(), _lib.check, dev, how) for how in CASES[:3]}
    out.update({how: _through_training(training, dev, how) for how in CASES[3:]})
    return out


def _where(a, b):
    """the first differing (tensor size, element) pairs of two concatenated arrays, for the message"""
    off = np.concatenate([[0], np.cumsum(oc.SIZES + (300,))])
    bad = np.nonzero(a != b)[0][:4]
    return [((oc.SIZES + ("stat",))[int(np.searchsorted(off, i, side="right")) - 1], int(i)) for i in bad]


def _assert_equalities(runs):
    for a, b, whats in EQUAL:
        for what in whats:
            assert np.array_equal(runs[a][what], runs[b][what]), (a, b, what, _where(runs[a][what], runs[b][what]))


@pytest.fixture(scope="module")
def parent():
    return np.load(FIXTURE)


@pytest.fixture(scope="module")
def runs():
    return _runs()


@pytest.mark.parametrize("how", CASES)
def test_adam_is_the_parents_bits(parent, runs, how):
    assert len(str(parent["parent"])) == 40
    got = runs[how]
    assert sorted(got) == (["ema", "m", "p", "v"] if how == "adam_three_ema" else ["m", "p", "v"])
    for what, a in got.items():
        want = parent["%s.%s" % (how, what)]
        assert a.dtype == want.dtype == np.uint32 and a.shape == want.shape == (sum(oc.SIZES) + (300 if what == "ema" else 0),)
        assert np.array_equal(a, want), (how, what, int((a != want).sum()), _where(a, want))


def test_the_entries_agree_with_each_other(parent, runs):
    """yf_train_adam_multi and its pinned form against yf_train_adam_step, step(ema=) against step(): here and in the recorded parent"""
    _assert_equalities(runs)
    _assert_equalities({how: {what: parent["%s.%s" % (how, what)] for what in ("p", "m", "v")} for how in CASES})
    start = _bits([torch.from_numpy(a) for a in oc.parameters(SEED)])
    for how in CASES:
        assert (runs[how]["p"] != start).sum() > sum(oc.SIZES) - 2 * len(oc.SIZES), how      # (the steps did something, to every tensor)


def _write(commit):
    sys.path.insert(0, ROOT)
    runs = _runs()
    _assert_equalities(runs)
    out = {"parent": np.array(commit)}
    for how, got in runs.items():
        for what, a in got.items():
            out["%s.%s" % (how, what)] = a
            print(how, what, a.shape, "%08x" % int(np.bitwise_xor.reduce(a)))
    np.savez(FIXTURE, **out)
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--write" and len(sys.argv[2]) == 40, __doc__
    _write(sys.argv[2])
