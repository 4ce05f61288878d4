"""training.SGD, training.Adam(weight_decay), training.param_groups, train_step(branch_weight) and train()'s opt-in train_params keys on
the GPU (`python -m pytest tests -m gpu`; csrc/yf_train_opt_kernels.h: tsgd_group_kernel / tadam_group_kernel behind
yf_train_opt_multi_pinned).

  * SGD bit for bit against torch.optim.SGD on the CPU, run here: parameters and momentum buffers after every step, over the
    configurations, sizes and layouts of tests/optim_cases.py, fresh and after load_state_dict of the CPU optimizer's state;
  * Adam with weight decay within test_adam_matches_torch's bound; Adam without it bit for bit yf_train_adam_multi_pinned;
  * one C call per step() whatever the number of groups, no table upload for an lr edit;
  * the three yolov5 groups on the real network; two SGD steps of the whole network on the reference's gradients, bit for bit;
  * branch_weight: linear in the heads, and [1, 1] / None leave every bit as it was; train() reads the keys only when asked to."""
import copy
import ctypes
import logging
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import optim_cases as oc  # noqa: E402
import voc_tree  # noqa: E402

WEIGHTS = os.path.join(ROOT, "yolo-fastest-and-embedded-deployment_amd", "assets", "weights", "yolo_fastest_256x320_epoch28.pth")
LOG = logging.getLogger("test-gpu-optim")


@pytest.fixture(scope="module")
def yf():
    import yolo_fastest_amd
    return yolo_fastest_amd


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _pair(arrays, dev):
    """the same values as CPU and as GPU Parameters"""
    return ([torch.nn.Parameter(torch.from_numpy(a.copy())) for a in arrays],
            [torch.nn.Parameter(torch.from_numpy(a.copy()).to(dev)) for a in arrays])


def _set_grads(ref, our, gs, dev):
    for r, o, g in zip(ref, our, gs):
        r.grad = None if g is None else torch.from_numpy(g.copy())
        o.grad = None if g is None else torch.from_numpy(g.copy()).to(dev)


def _same_bits(our, ref, what):
    a, b = oc.bits(our.detach().cpu().numpy()), oc.bits(ref.detach().numpy())
    assert np.array_equal(a, b), (what, int((a != b).sum()), np.nonzero(a != b)[0][:4].tolist())


# ---- SGD, bits ----
@pytest.mark.parametrize("resume", [False, True])
@pytest.mark.parametrize("which", ["one", "three"])
@pytest.mark.parametrize("cfg", oc.CONFIGS)
def test_sgd_is_torchs_bit_for_bit(yf, dev, cfg, which, resume):
    """Five steps: the six sizes in one optimizer (one group, or three with their own lr and weight_decay, the 257-element tensor alone in
    the middle one), element 0 of every parameter and gradient -0.0, gradients 1e-6 .. 10, an lr edit before step 3, one tensor whose
    first gradient arrives at step 2.  `resume`: our optimizer starts at step 3 from the CPU optimizer's state_dict."""
    from yolo_fastest_amd import training
    mom, nesterov, wd = cfg
    groups = oc.layout(which, wd)
    ref, our = _pair(oc.parameters(3), dev)

    def spec(ps):
        return [dict(params=[ps[i] for i in idx], lr=lr, weight_decay=w) for idx, lr, w in groups]
    o_ref = torch.optim.SGD(spec(ref), lr=0.01, momentum=mom, nesterov=nesterov)
    o_our = training.SGD(spec(our), lr=0.01, momentum=mom, nesterov=nesterov)
    for it in range(oc.STEPS):
        gs = oc.gradients(3, it)
        if resume and it < 2:
            _set_grads(ref, ref, gs, "cpu")
            o_ref.step()
            if it == 1:
                with torch.no_grad():
                    for r, o in zip(ref, our):
                        o.copy_(r)
                o_our.load_state_dict(copy.deepcopy(o_ref.state_dict()))
                assert mom == 0 or all(o_our.state[o]["momentum_buffer"].is_cuda for o in our)
            continue
        if it == 2:
            for grp in o_ref.param_groups + o_our.param_groups:
                grp["lr"] = grp["lr"] * oc.LR_EDIT
        _set_grads(ref, our, gs, dev)
        o_ref.step(); o_our.step()
        for n, r, o in zip(oc.SIZES, ref, our):
            _same_bits(o, r, ("parameter", it, n))
            buf = o_ref.state[r].get("momentum_buffer") if r in o_ref.state else None
            mine = o_our.state[o].get("momentum_buffer") if o in o_our.state else None
            assert (buf is None) == (mine is None), (it, n)
            if buf is not None:
                _same_bits(mine, buf, ("momentum_buffer", it, n))
    assert mom == 0 or resume or o_our.state[our[oc.LATE]]["momentum_buffer"] is not None


def test_sgd_has_no_cpu_path(yf, dev):
    from yolo_fastest_amd import training
    cpu = torch.nn.Parameter(torch.zeros(3)); cpu.grad = torch.ones(3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        training.SGD([cpu], lr=0.1).step()
    half = torch.nn.Parameter(torch.zeros(3, device=dev, dtype=torch.float16)); half.grad = torch.ones_like(half)
    with pytest.raises(RuntimeError, match="float32"):
        training.SGD([half], lr=0.1).step()


def test_sgd_follows_lambda_lr(yf, dev):
    """lr_scheduler.LambdaLR on training.SGD as on torch's: the same parameters, bit for bit, over four scheduled steps."""
    from torch.optim import lr_scheduler
    from yolo_fastest_amd import training
    ref, our = _pair(oc.parameters(5), dev)
    o_ref = torch.optim.SGD(ref, lr=0.01, momentum=0.937, nesterov=True, weight_decay=5e-4)
    o_our = training.SGD(our, lr=0.01, momentum=0.937, nesterov=True, weight_decay=5e-4)
    s_ref, s_our = [lr_scheduler.LambdaLR(o, lr_lambda=lambda e: training.cosine_factor(e, 4)) for o in (o_ref, o_our)]
    for it in range(4):
        _set_grads(ref, our, oc.gradients(5, it + 1), dev)
        o_ref.step(); o_our.step()
        s_ref.step(); s_our.step()
        assert o_ref.param_groups[0]["lr"] == o_our.param_groups[0]["lr"]
        for n, r, o in zip(oc.SIZES, ref, our):
            _same_bits(o, r, (it, n))


# ---- Adam ----
def test_adam_with_weight_decay_matches_torch(yf, dev):
    """Five steps against torch.optim.Adam(betas=(0.937, 0.999)) on the CPU within test_adam_matches_torch's bound, 2e-7 (it + 1): three
    groups of which only the middle one decays (5e-4), the sizes of the SGD test, an lr edit before step 3."""
    from yolo_fastest_amd import training
    groups = [((0, 1, 2), 0.001, 0.0), ((4, 5), 0.0005, 5e-4), ((3,), 0.002, 0.0)]
    ref, our = _pair(oc.parameters(7), dev)

    def spec(ps):
        return [dict(params=[ps[i] for i in idx], lr=lr, weight_decay=w) for idx, lr, w in groups]
    o_ref = torch.optim.Adam(spec(ref), lr=0.001, betas=(0.937, 0.999), eps=1e-08)
    o_our = training.Adam(spec(our), lr=0.001, betas=(0.937, 0.999), eps=1e-08)
    assert [g["weight_decay"] for g in o_our.param_groups] == [0.0, 5e-4, 0.0]
    for it in range(oc.STEPS):
        gs = [g if g is not None else np.zeros(oc.SIZES[oc.LATE], np.float32) for g in oc.gradients(7, it)]
        if it == 2:
            for grp in o_ref.param_groups + o_our.param_groups:
                grp["lr"] = grp["lr"] * oc.LR_EDIT
        _set_grads(ref, our, gs, dev)
        o_ref.step(); o_our.step()
        for n, r, o in zip(oc.SIZES, ref, our):
            err = np.abs(o.detach().cpu().numpy() - r.detach().numpy()).max()
            print("adam + decay: step %d, %4d elements: max |d| %.2e" % (it + 1, n, err))
            assert err <= 2e-7 * (it + 1), (it, n, err)
    # the decay is really applied, and only to the middle group: against a CPU run without it
    plain = [torch.nn.Parameter(torch.from_numpy(a.copy())) for a in oc.parameters(7)]
    o_plain = torch.optim.Adam([dict(params=[plain[i] for i in idx], lr=lr) for idx, lr, _ in groups], lr=0.001, betas=(0.937, 0.999), eps=1e-08)
    for it in range(oc.STEPS):
        gs = [g if g is not None else np.zeros(oc.SIZES[oc.LATE], np.float32) for g in oc.gradients(7, it)]
        if it == 2:
            for grp in o_plain.param_groups:
                grp["lr"] = grp["lr"] * oc.LR_EDIT
        _set_grads(plain, plain, gs, "cpu")
        o_plain.step()
    assert np.abs(our[5].detach().cpu().numpy() - plain[5].detach().numpy()).max() > 1e-5
    assert np.abs(our[3].detach().cpu().numpy() - plain[3].detach().numpy()).max() <= 1e-6


def test_adam_without_decay_keeps_the_bits_of_adam_multi(yf, dev):
    """training.Adam (one group, weight_decay 0: the grouped kernel) against a direct call of yf_train_adam_multi_pinned on the same
    inputs: p, exp_avg and exp_avg_sq bit-equal after each of 3 steps."""
    from yolo_fastest_amd import _lib, training
    lib = _lib.lib()
    arrays = oc.parameters(11)
    our = [torch.nn.Parameter(torch.from_numpy(a.copy()).to(dev)) for a in arrays]
    p = [torch.from_numpy(a.copy()).to(dev) for a in arrays]
    m, v = [torch.zeros_like(t) for t in p], [torch.zeros_like(t) for t in p]
    n = len(p)
    opt = training.Adam(our, lr=0.001, betas=(0.9, 0.999), eps=1e-08)
    table = torch.empty(48 * n, dtype=torch.uint8, device=dev)

    def arr(ts):
        return (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
    for it in range(3):
        gs = [torch.from_numpy(g).to(dev) for g in oc.gradients(11, it + 1)]
        for o, g in zip(our, gs):
            o.grad = g.clone()
        lr = 0.001 if it < 2 else 0.00037
        opt.param_groups[0]["lr"] = lr
        opt.step()
        _lib.check(lib.yf_train_adam_multi_pinned(dev.index, n, arr(p), arr(gs), arr(m), arr(v), (ctypes.c_long * n)(*[t.numel() for t in p]), lr, 0.9,
                                                  0.999, 1e-08, it + 1, table.data_ptr(), table.numel(), None, 1,
                                                  ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        torch.cuda.synchronize()
        for i, o in enumerate(our):
            st = opt.state[o]
            for got, want, what in ((o, p[i], "p"), (st["exp_avg"], m[i], "exp_avg"), (st["exp_avg_sq"], v[i], "exp_avg_sq")):
                assert np.array_equal(oc.bits(got.detach().cpu().numpy()), oc.bits(want.cpu().numpy())), (it, oc.SIZES[i], what)


# ---- one launch per step ----
OPT_ENTRIES = ("yf_train_opt_multi_pinned", "yf_train_adam_multi_pinned", "yf_train_adam_multi", "yf_train_adam_step")
UPLOAD_ARG = {"yf_train_opt_multi_pinned": 15, "yf_train_adam_multi_pinned": 15}


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_a_step_of_three_groups_is_one_call(yf, dev, monkeypatch, kind):
    """Counting callables in place of the C entries on the library object: a three-group step() is exactly one optimizer call, and a step
    that differs from the one before only in lr uploads no table (SGD's second step does: the first-step marks fall)."""
    from yolo_fastest_amd import _lib, training
    lib = _lib.lib()
    calls = []
    for name in OPT_ENTRIES:
        def counting(*a, _orig=getattr(lib, name), _name=name):
            calls.append((_name, a[UPLOAD_ARG[_name]] if _name in UPLOAD_ARG else None))
            return _orig(*a)
        monkeypatch.setattr(lib, name, counting)
    our = [torch.nn.Parameter(torch.from_numpy(a.copy()).to(dev)) for a in oc.parameters(13)]
    spec = [dict(params=[our[i] for i in idx], lr=lr, weight_decay=w) for idx, lr, w in oc.layout("three", 5e-4)]
    opt = training.SGD(spec, lr=0.01, momentum=0.937, nesterov=True) if kind == "sgd" else training.Adam(spec, lr=0.001, betas=(0.937, 0.999))
    for o, g in zip(our, oc.gradients(13, 1)):
        o.grad = torch.from_numpy(g).to(dev)                          # the same gradient tensors in every step, like the trainer's flat buffer
    for it in range(4):
        for grp in opt.param_groups:
            grp["lr"] = grp["lr"] * 0.9                                   # the warm-up's per-iteration edit
        before = len(calls)
        opt.step()
        assert [c[0] for c in calls[before:]] == ["yf_train_opt_multi_pinned"], (it, calls[before:])
    torch.cuda.synchronize()
    uploads = [c[1] for c in calls]
    assert uploads[0] == 1 and uploads[2:] == [0, 0], uploads
    assert uploads[1] == (1 if kind == "sgd" else 0), uploads
    assert all(torch.isfinite(o).all() for o in our)


# ---- the groups on the real network ----
def test_param_groups_on_the_network(yf, dev):
    from yolo_fastest_amd import training
    m = yf.YoloFastest(yf.io_params_for(256)).to(dev)
    g = training.param_groups(m, 5e-4)
    bn, w, b = [], [], []
    for _, mod in m.named_modules():                                    # yolov5's rule, restated
        if isinstance(mod, torch.nn.BatchNorm2d):
            bn.append(mod.weight)
        elif isinstance(mod, (torch.nn.Conv2d, torch.nn.ConvTranspose2d)):
            w.append(mod.weight)
        if getattr(mod, "bias", None) is not None:
            b.append(mod.bias)
    assert len(g) == 3 and "weight_decay" not in g[0] and g[1]["weight_decay"] == 5e-4 and "weight_decay" not in g[2]
    for got, want in zip(g, (bn, w, b)):
        assert len(got["params"]) == len(want) > 0 and all(x is y for x, y in zip(got["params"], want))
    ids = [id(p) for d in g for p in d["params"]]
    assert len(ids) == len(set(ids)) == 256 and set(ids) == {id(p) for p in m.parameters()}
    assert all(p.is_cuda for d in g for p in d["params"])


def _split(flat, sizes):
    off = np.concatenate([[0], np.cumsum(sizes)])
    return [flat[off[i]:off[i + 1]] for i in range(len(sizes))]


def test_two_teacher_forced_sgd_iterations_of_the_network(yf, golden, dev):
    """The shipped checkpoint's 326 k parameters, the reference's gradients of its two iterations (golden_train_256.npz) in p.grad,
    yolov5's three groups: training.SGD against torch.optim.SGD on a CPU copy, every parameter bit-equal after both steps."""
    from yolo_fastest_amd import training
    gt = golden("golden_train_256")
    io = yf.io_params_for(256)
    m = yf.YoloFastest(io).to(dev)
    m.load_state_dict(torch.load(WEIGHTS, map_location=dev))
    c = yf.YoloFastest(io)
    c.load_state_dict(torch.load(WEIGHTS, map_location="cpu"))
    assert [n for n, _ in m.named_parameters()] == [str(s) for s in gt["param_names"]]
    o_our = training.SGD(training.param_groups(m, 5e-4), lr=0.01, momentum=0.937, nesterov=True)
    o_ref = torch.optim.SGD(training.param_groups(c, 5e-4), lr=0.01, momentum=0.937, nesterov=True)
    start = [q.detach().clone() for q in c.parameters()]
    total = 0
    for it in (1, 2):
        for p, q, g in zip(m.parameters(), c.parameters(), _split(gt["grads_%d" % it], gt["param_sizes"])):
            g = torch.from_numpy(np.ascontiguousarray(g.reshape(tuple(q.shape))))
            q.grad, p.grad = g.clone(), g.to(dev)
        o_our.step(); o_ref.step()
        total = 0
        for (name, p), q in zip(m.named_parameters(), c.parameters()):
            _same_bits(p, q, (it, name))
            total += p.numel()
    assert total > 326000
    assert max(float((q.detach() - w).abs().max()) for q, w in zip(c.parameters(), start)) > 1e-4      # (the steps did something)


# ---- branch_weight ----
class _NoStep:
    """train_step's optimizer, without the update: every pass below sees the same parameters"""

    def __init__(self, params):
        self.params = list(params)

    def zero_grad(self):
        for p in self.params:
            p.grad = None

    def step(self):
        pass


def _vals(losses):
    return [float(v.detach()) if torch.is_tensor(v) else float(v) for v in losses]


@pytest.fixture(scope="module")
def branch(yf, golden, dev):
    """One iteration of the shipped checkpoint on the training golden's batch, five times without an update in between (train-mode
    BatchNorm uses batch statistics, so every pass is the same forward): a plain train_step, branch_weight None, [1, 1] and [0.5, 2.0],
    and one backward per head alone.  Each pass: (the seven values, every p.grad)."""
    from yolo_fastest_amd import training, validation as val
    gt = golden("golden_train_256")
    io = yf.io_params_for(256)
    m = yf.YoloFastest(io).to(dev)
    m.load_state_dict(torch.load(WEIGHTS, map_location=dev))
    m.train()
    x = ((torch.from_numpy(gt["input_u8"].astype(np.float32))[:, None] - 128.0) / 255.0).to(dev)
    targets = torch.from_numpy(gt["targets"]).to(dev)
    crit = [val.YOLOLossV3(io["anchors"][i], io["num_cls"], io["input_shape"], dev, model=m) for i in range(2)]
    opt = _NoStep(m.parameters())

    def grads():
        return [p.grad.detach().clone() for p in m.parameters()]
    out = dict(names=[n for n, _ in m.named_parameters()], zero=(gt["grad_absmax_f64"] < 1e-9).tolist(), step=lambda bw: training.train_step(m, crit, opt, x, targets, branch_weight=bw))
    out["plain"] = (training.train_step(m, crit, opt, x, targets), grads())
    for key, bw in (("none", None), ("ones", [1.0, 1.0]), ("weighted", [0.5, 2.0])):
        out[key] = (training.train_step(m, crit, opt, x, targets, branch_weight=bw), grads())
    for i, key in enumerate(("large", "small")):
        opt.zero_grad()
        pred = m(x)
        v = crit[i](pred[i], targets)
        v[0].backward()
        out[key] = (v, grads())
    return out


@pytest.mark.parametrize("key", ["none", "ones"])
def test_branch_weight_of_ones_or_none_keeps_every_bit(branch, key):
    (want, g_want), (got, g_got) = branch["plain"], branch[key]
    assert torch.equal(got[0].detach(), want[0].detach()) and _vals(got) == _vals(want)
    for name, a, b in zip(branch["names"], g_got, g_want):
        assert np.array_equal(oc.bits(a.cpu().numpy()), oc.bits(b.cpu().numpy())), name


def test_branch_weight_scales_each_heads_losses(branch):
    """[0.5, 2.0]: losses[j] = 0.5 l_large[j] + 2.0 l_small[j] from the per-head values obtained here, exactly (the factors are powers
    of two).  For the same reason the layers only one head reaches -- where the other head's single pass leaves an all-zero gradient --
    carry exactly that head's gradient times its factor."""
    (l_large, g_large), (l_small, g_small), (got, g_got) = branch["large"], branch["small"], branch["weighted"]
    assert torch.equal(got[0].detach(), l_large[0].detach() * 0.5 + l_small[0].detach() * 2.0)
    assert _vals(got)[1:] == [0.5 * float(a) + 2.0 * float(b) for a, b in zip(l_large[1:], l_small[1:])]
    private = 0
    for name, g, gl, gs in zip(branch["names"], g_got, g_large, g_small):
        if not gs.any() or not gl.any():
            private += 1
            assert torch.equal(g, 0.5 * gl + 2.0 * gs), name
    assert private >= 30                                                    # deconv5_1, conv4_1_1..5, head_4; conv5_3..6, head_5
    with pytest.raises(ValueError, match="branch_weight"):
        branch["step"]([1.0])


def test_branch_weight_gradients_are_linear_in_the_heads(branch):
    """[0.5, 2.0]: every p.grad against 0.5 gL + 2.0 gS, gL and gS from two single-head passes of our own backward -- a linearity check,
    at 2 fp32 ulps of the tensor's largest element (one rounding per product and one for the sum).

    One backward of the weighted sum of the head gradients does not meet this in the layers both heads reach: backward(a + b) and
    backward(a) + backward(b) round differently at every accumulation of the fp32 backward, not once (measured with that form: median
    7.6 ulp over the 256 tensors, worst 156 ulp among those whose exact gradient is not zero, and anything at all in the 23 BatchNorm
    biases whose exact gradient is zero).  train_step therefore takes the heads back one at a time and lets p.grad accumulate, which is
    the expression above term by term."""
    (_, g_large), (_, g_small), (_, g_got) = branch["large"], branch["small"], branch["weighted"]
    rows = []
    for name, g, gl, gs in zip(branch["names"], g_got, g_large, g_small):
        want = 0.5 * gl.double() + 2.0 * gs.double()
        ulp = float(np.spacing(np.float32(want.abs().max().item())))
        rows.append((float((g.double() - want).abs().max()) / ulp, name))
    over = [r for r in rows if r[0] > 2]
    real = [r for r, z in zip(rows, branch["zero"]) if not z]                 # (the rest: gradients that are zero in exact arithmetic)
    print("branch_weight [0.5, 2.0] vs 0.5 gL + 2.0 gS, in fp32 ulps of each tensor's largest element: median %.2f, %d of %d tensors above 2; "
          "worst %.1f (%s) among the %d tensors whose exact gradient is not zero, %.3g (%s) among all"
          % (float(np.median([r[0] for r in rows])), len(over), len(rows), max(real)[0], max(real)[1], len(real), max(rows)[0], max(rows)[1]))
    assert not over, sorted(over, reverse=True)[:5]


# ---- train() ----
def test_train_reads_the_keys_only_when_asked(yf, dev, tmp_path):
    """On the bundled VOC tree, one epoch of 2 iterations at batch 4 from the shipped checkpoint: optimizer="sgd", branch_weight=True runs
    and writes its checkpoint; optimizer=None twice from one seed gives identical state-dicts (with train_params' momentum, weight_decay
    and branch_weight set to something else in the second run: the default reads none of them); optimizer="adam" gives another."""
    import random
    from yolo_fastest_amd import training
    from yolo_fastest_amd.dataset import DetectDataset
    trees = voc_tree.make_trees(tmp_path)

    def run(tag, tp=(), **kw):
        params = copy.deepcopy(yf.config_params)
        params["io_params"]["save_path"] = str(tmp_path / tag)
        params["augment_params"] = voc_tree.aug_params(trees)
        params["train_params"].update(total_epochs=1, batch_size=4, pretrained_pth=WEIGHTS)
        params["train_params"].update(dict(tp))
        ds = DetectDataset([256, 320, 1], [512, 640, 3], LOG, aug_params=params["augment_params"], max_boxes=64, device=dev)
        ds.img_list = sorted(ds.img_list)[:8]                            # 2 iterations
        assert len(ds) == 8
        torch.manual_seed(0)
        random.seed(0)
        training.train(params, dev, None, train_dataset=ds, logger=LOG, **kw)
        path = os.path.join(params["io_params"]["save_path"], "YOLO-Fastest_epoch_0.pth")
        assert os.path.exists(path)
        return torch.load(path, map_location="cpu")

    def same(a, b):
        return all(torch.equal(a[k], b[k]) for k in a)
    sgd = run("sgd", tp=dict(branch_weight=[0.5, 2.0]), optimizer="sgd", branch_weight=True)      # (one backward per head inside train())
    assert len(sgd) == 508 and all(torch.isfinite(v).all() for v in sgd.values())
    ref1 = run("ref1")
    ref2 = run("ref2", tp=dict(momentum=0.5, weight_decay=0.1, branch_weight=[3.0, 0.25]))
    assert same(ref1, ref2)
    adam = run("adam", optimizer="adam")
    assert not same(ref1, adam) and not same(ref1, sgd)
    assert int(adam["conv0.1.num_batches_tracked"]) == int(ref1["conv0.1.num_batches_tracked"])
    with pytest.raises(ValueError, match="branch_weight"):
        run("bad", tp=dict(branch_weight=[1.0]), branch_weight=True)
