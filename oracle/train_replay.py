"""ORACLE (test infrastructure, not product): the training step's backward replayed on a tape of the forward that was actually run.

A from-the-input float64 backward cannot be compared tightly with an fp32 one: a ReLU decision within rounding of zero falls on the
other side in fp32 and moves everything upstream of it by a percent (tests/test_gpu_training.py, tests/flip_reach.py).  Here the
float64 backward is LINEARISED AT THE TAPE instead: every unit's input value is the tape's, the conv output in front of BatchNorm is
the tape's, the ReLU is multiplication by the tape's (y > 0).  Nothing the fp32 forward decided can differ then, and the gradients
agree with an fp32 backward to rounding of sums (1e-6 relative to a tensor's largest element, not 4e-3).

  make_tape(sd, x, dtype)                      the oracle's own train-mode forward, recorded like training.train_forward records it
  replay(sd, tape, g_hl, g_hs, dtype, ...)     one torch-autograd pass over backbone_oracle.forward's graph -> (gradients, forward errors)
  compare(g_dev, g64, g_twin)                  the acceptance rule, in one place

The tape is what `training.train_forward(model, x)` returns: per unit (x, z, y, stats, relu, geom) -- z the conv output, y the unit's
output (conv3 of a BasicResBlock: with the residual already added, as the device adds it in place) -- and per head its input.
Only tests/ import this file.
"""
import numpy as np
import torch
import torch.nn.functional as F

from . import backbone_oracle as bo

_RES = lambda n: [n + ".conv1", n + ".conv2", n + ".conv3"]                       # noqa: E731
# the trunk of backbone_oracle.forward up to the first branch point (conv4_2), element by element
_TRUNK = (["conv0", "conv1_2", "conv1_3", "conv1_4", "res1_1", "conv1_8", "conv1_9", "conv2_1", "res2_1", "res2_2", "conv2_2", "conv2_3",
           "conv3_1", "res3_1", "res3_2", "conv3_2", "conv3_3", "conv3_4", "res3_3", "res3_4", "res3_5", "res3_6", "conv3_5", "conv3_6",
           "conv4_1", "res4_1", "res4_2", "res4_3", "res4_4", "conv4_2"])
_SEQ2 = ["conv4_3", "conv5_1", "res5_1", "res5_2", "res5_3", "res5_4", "res5_5", "conv5_2"]
_SEQ3 = ["conv5_3", "conv5_4", "conv5_5", "conv5_6"]
_SEQ4 = ["conv4_1_1", "conv4_1_2", "conv4_1_3", "conv4_1_4", "conv4_1_5"]

ZERO_CAP = 27          # at most this many tensors may be left out of the relative comparison as "zero in exact arithmetic"
ZERO_REL = 1e-9        # ... a tensor whose float64 gradient is below this fraction of the LARGEST float64 gradient (they sit at 1e-16)


def _units_of(elem):
    return _RES(elem) if elem.startswith("res") else [elem]


def unit_names(first_unit=None):
    """The conv+BN units the replay visits, in forward order (with `first_unit`: from that unit on)."""
    trunk = list(_TRUNK)
    if first_unit is not None:
        starts = [_units_of(e)[0] for e in trunk]
        if first_unit not in starts:
            raise ValueError("first_unit must open an element of the trunk (a plain unit or a block's conv1), got %r" % (first_unit,))
        trunk = trunk[starts.index(first_unit):]
    out = []
    for e in trunk + _SEQ2 + _SEQ3 + ["deconv5_1"] + _SEQ4:
        out += _units_of(e)
    return out


def parameter_keys(first_unit=None):
    keys = []
    for u in unit_names(first_unit):
        keys += [u + ".0.weight", u + ".1.weight", u + ".1.bias"]
    return keys + ["head_4.weight", "head_4.bias", "head_5.weight", "head_5.bias"]


def _conv(sd, name, x):
    _, kind, cin, cout, k, s, relu = bo._BY_NAME[name]
    w = sd[name + ".0.weight"]
    if kind == "dc":
        return F.conv_transpose2d(x, w, None, stride=2, padding=0)
    return F.conv2d(x, w, None, stride=s, padding=(k - 1) // 2, groups=(x.shape[1] if kind == "dw" else 1))


def _walk(unit, head, x, first_unit=None):
    """backbone_oracle.forward's graph (yolo_fastest.py:150-218).  unit(name, x, residual_of) -> (y, x as the unit used it);
    head(name, x) -> logits.  x None: the walk starts at `first_unit`, whose input the callback supplies."""
    def run(elems, x):
        for e in elems:
            if e.startswith("res"):
                y, xin = unit(e + ".conv1", x, None)
                y, _ = unit(e + ".conv2", y, None)
                x, _ = unit(e + ".conv3", y, xin)              # out += residual, the block's input as conv1 saw it
            else:
                x, _ = unit(e, x, None)
        return x
    trunk = list(_TRUNK)
    if first_unit is not None:
        trunk = trunk[[_units_of(e)[0] for e in trunk].index(first_unit):]
    a = run(trunk, x)                                          # conv4_2
    b = run(_SEQ2, a)                                          # conv5_2
    c = run(_SEQ3, b)
    hs = head("head_5", c)
    d, _ = unit("deconv5_1", b, None)
    e = run(_SEQ4, torch.cat((a, d), 1))
    hl = head("head_4", e)
    return hl, hs


def make_tape(sd, x, dtype=torch.float64):
    """The oracle's train-mode forward in `dtype`, recorded in the layout of training.train_forward -> (head_large, head_small, tape).
    The running statistics of `sd` are not touched."""
    sd = {k: v.detach().to(dtype) for k, v in sd.items() if v.is_floating_point()}
    tape = {}

    def unit(name, x, res):
        relu = bo._BY_NAME[name][6]
        z = _conv(sd, name, x)
        y = F.batch_norm(z, None, None, sd[name + ".1.weight"], sd[name + ".1.bias"], True, 0.0, bo.BN_EPS)
        y = F.relu(y) if relu else y
        if res is not None:
            y = y + res
        tape[name] = (x, z, y, None, int(relu), None)
        return y, x

    def head(name, x):
        tape[name] = x
        return F.conv2d(x, sd[name + ".weight"], sd[name + ".bias"])
    with torch.no_grad():
        hl, hs = _walk(unit, head, x.to(dtype))
    return hl, hs, tape


class _ShortSumsBN(torch.autograd.Function):
    """DEFECT MODEL for the sensitivity tests: train-mode BatchNorm whose backward takes its two sums per channel (sum dy, sum dy xhat)
    without the last four columns of every plane -- a ragged last block that was never summed."""

    @staticmethod
    def forward(ctx, z, gamma, beta):
        mu = z.mean((0, 2, 3), keepdim=True)
        inv = (z.var((0, 2, 3), unbiased=False, keepdim=True) + bo.BN_EPS).rsqrt()
        xhat = (z - mu) * inv
        ctx.save_for_backward(xhat, inv, gamma)
        return xhat * gamma[None, :, None, None] + beta[None, :, None, None]

    @staticmethod
    def backward(ctx, dy):
        xhat, inv, gamma = ctx.saved_tensors
        m = dy.shape[0] * dy.shape[2] * dy.shape[3]
        s1 = dy[..., :-4].sum((0, 2, 3))
        s2 = (dy * xhat)[..., :-4].sum((0, 2, 3))
        dx = gamma[None, :, None, None] * inv * (dy - s1[None, :, None, None] / m - xhat * s2[None, :, None, None] / m)
        return dx, s2, s1


def replay(sd, tape, g_hl, g_hs, dtype=torch.float64, first_unit=None, defect=None):
    """One torch-autograd pass over the oracle's graph on the CPU in `dtype`, linearised at `tape` -> (grads, fwd_err).

    Per unit: the input VALUE is the tape's x (gradient still flows to whatever produced it), the conv output in front of BatchNorm is the
    tape's z (so the tape's conv rounding does not enter the statistics), BatchNorm uses batch statistics computed in `dtype` from that
    z, ReLU is multiplication by the tape's (y > 0).  Residual adds, the concat, the deconv, the two branch points and the two head
    convs are backbone_oracle.forward's.  (The substitution is written `x_tape + (x - x.detach())`: the same value and gradient as
    `x + (x_tape - x).detach()`, but exactly x_tape in every number format.)

    grads: {parameter key: gradient} for the replayed units and both heads.  first_unit: start at that unit's tape input; only the units
    from there on are replayed.  fwd_err: {unit: (max|z_tape - conv(x_tape)| / max|z_tape|, max|y_tape - act(bn(z_tape))| / max|y_tape|)}
    evaluated in `dtype` -- in float64 that holds every conv and BatchNorm forward of the pass to the operator level.

    defect (sensitivity tests only): {"drop_skip": block} the block's skip gradient is lost; {"short_sums": unit} that unit's BatchNorm
    backward sums miss the last four columns of every plane; {"own_mask": (unit, shift)} that unit's mask is recomputed from the
    replay's own pre-activation, against a y that was shifted by `shift`."""
    defect = defect or {}
    dt = dtype
    P = {k: sd[k].detach().to("cpu", dt).clone().requires_grad_(True) for k in parameter_keys(first_unit)}
    fwd_err = {}

    def cvt(t):
        return t.detach().to("cpu", dt)

    def sub(t_tape, t):
        return t_tape if t is None or not t.requires_grad else t_tape + (t - t.detach())

    def unit(name, x, res):
        xt, zt, yt, _, relu, _ = tape[name]
        x = sub(cvt(xt), x)
        c = _conv(P, name, x)
        zt = cvt(zt)
        ez = float((zt - c.detach()).abs().max() / zt.abs().max())
        z = zt + (c - c.detach())
        del c
        gamma, beta = P[name + ".1.weight"], P[name + ".1.bias"]
        if defect.get("short_sums") == name:
            y = _ShortSumsBN.apply(z, gamma, beta)
        else:
            y = F.batch_norm(z, None, None, gamma, beta, True, 0.0, bo.BN_EPS)
        yt = cvt(yt)
        want = F.relu(y.detach()) if relu else y.detach()
        if res is not None:
            want = want + res.detach()
        ey = float((yt - want).abs().max() / yt.abs().max())
        del want
        fwd_err[name] = (ez, ey)
        if relu:
            mask = yt > 0
            if defect.get("own_mask", (None,))[0] == name:
                mask = (y.detach() - defect["own_mask"][1]) > 0
            y = y * mask.to(dt)
        if res is not None:
            y = y + (res.detach() if defect.get("drop_skip") == name[:-len(".conv3")] else res)
        return y, x

    def head(name, x):
        return F.conv2d(sub(cvt(tape[name]), x), P[name + ".weight"], P[name + ".bias"])
    with torch.enable_grad():
        hl, hs = _walk(unit, head, None, first_unit) if first_unit is not None else _walk(unit, head, cvt(tape["conv0"][0]))
        keys = list(P)
        g = torch.autograd.grad([hl, hs], [P[k] for k in keys], [cvt(g_hl), cvt(g_hs)])
    return dict(zip(keys, g)), fwd_err


class Comparison:
    """What compare() found: .failures (empty = accepted), per-tensor errors, the figures to print."""

    def __init__(self):
        self.failures, self.e_dev, self.e_twin, self.zero = [], {}, {}, []
        self.zero_dev = self.zero_twin = 0.0

    @property
    def ok(self):
        return not self.failures

    def figures(self):
        d, t = np.array(list(self.e_dev.values())), np.array(list(self.e_twin.values()))
        return dict(dev_median=float(np.median(d)), dev_p90=float(np.quantile(d, 0.9)), dev_max=float(d.max()),
                    twin_median=float(np.median(t)), twin_p90=float(np.quantile(t, 0.9)), twin_max=float(t.max()),
                    zero=len(self.zero), zero_dev=self.zero_dev, zero_twin=self.zero_twin)

    def table(self, worst=5):
        f = self.figures()
        rows = ["%d tensors + %d zero in exact arithmetic: device median %.2e / p90 %.2e / max %.2e; fp32 twin median %.2e / p90 %.2e / max %.2e; "
                "zero set: device %.2e, twin %.2e" % (len(self.e_dev), f["zero"], f["dev_median"], f["dev_p90"], f["dev_max"], f["twin_median"],
                                                      f["twin_p90"], f["twin_max"], f["zero_dev"], f["zero_twin"])]
        med = f["twin_median"]
        order = sorted(self.e_dev, key=lambda k: -self.e_dev[k] / max(self.e_twin[k], med))
        for k in order[:worst]:
            rows.append("  %-28s device %.2e  twin %.2e  (%.1fx of its bound's base)" % (k, self.e_dev[k], self.e_twin[k],
                                                                                        self.e_dev[k] / max(self.e_twin[k], med)))
        return "\n".join(rows + ["  FAIL " + s for s in self.failures])


def compare(g_dev, g64, g_twin, ratio=2.0, per_tensor=8.0, zero_ratio=8.0):
    """The acceptance rule for gradients `g_dev` against the float64 replay `g64` of their own tape, with the same replay in float32 on
    the CPU (`g_twin`: torch's own fp32 arithmetic on exactly the linearisation the device used) as the yardstick.  Per kept tensor
    e = max|g - g64| / max|g64|.  Accepted when
      * median and 90th percentile of e_dev over the tensors are at most `ratio` x those of e_twin,
      * every tensor has e_dev[t] <= per_tensor * max(e_twin[t], median(e_twin)),
      * the tensors that are zero in exact arithmetic (at most ZERO_CAP, BatchNorm biases only) have max|g_dev| at most `zero_ratio` x
        the largest max|g_twin| over that set.
    The margins are for another summation order (another draw from the same rounding distribution), nothing else."""
    r = Comparison()
    keys = list(g64)
    assert set(keys) <= set(g_dev) and set(keys) <= set(g_twin)
    a64 = {k: float(g64[k].abs().max()) for k in keys}
    top = max(a64.values())
    for k in keys:
        d, t, w = (torch.as_tensor(g[k]).detach().to("cpu", torch.float64) for g in (g_dev, g_twin, g64))
        if d.shape != w.shape or not bool(torch.isfinite(d).all()):
            r.failures.append("%s: shape %s / non-finite" % (k, tuple(d.shape)))
            continue
        if a64[k] <= ZERO_REL * top:
            r.zero.append(k)
            r.zero_dev, r.zero_twin = max(r.zero_dev, float(d.abs().max())), max(r.zero_twin, float(t.abs().max()))
            continue
        r.e_dev[k] = float((d - w).abs().max()) / a64[k]
        r.e_twin[k] = float((t - w).abs().max()) / a64[k]
    if len(r.zero) > ZERO_CAP or any(not k.endswith(".1.bias") for k in r.zero):
        r.failures.append("%d tensors are zero in the float64 replay (cap %d, BatchNorm biases only): %s" % (len(r.zero), ZERO_CAP, r.zero))
    if r.zero and r.zero_dev > zero_ratio * r.zero_twin:
        r.failures.append("zero set: device %.3g > %g x twin %.3g" % (r.zero_dev, zero_ratio, r.zero_twin))
    if not r.e_dev:
        r.failures.append("nothing compared")
        return r
    d, t = np.array([r.e_dev[k] for k in r.e_dev]), np.array([r.e_twin[k] for k in r.e_dev])
    med = float(np.median(t))
    if np.median(d) > ratio * med:
        r.failures.append("median %.3g > %g x %.3g" % (np.median(d), ratio, med))
    if np.quantile(d, 0.9) > ratio * np.quantile(t, 0.9):
        r.failures.append("90th percentile %.3g > %g x %.3g" % (np.quantile(d, 0.9), ratio, np.quantile(t, 0.9)))
    for k in r.e_dev:
        if r.e_dev[k] > per_tensor * max(r.e_twin[k], med):
            r.failures.append("%s: %.3g > %g x max(%.3g, %.3g)" % (k, r.e_dev[k], per_tensor, r.e_twin[k], med))
    return r
