"""TEST INFRASTRUCTURE (CPU only, never imported by the product): the fp32-storage plans (`precision` "f32" and "f16x3") replayed ONE LAUNCH
AT A TIME against the plain float64 evaluation of that launch.

tests/f16_replay.py does this for the fp16-storage plan, whose unit is an fp16 ulp: anything below 2.4e-4 relative is invisible to it, and
the fp32 / split-operand plans run other kernels.  Here a launch has NO rounding point: fp32 storage keeps every tensor as the kernel computed
it, so the exact value of a launch is its float64 evaluation from the input tensor(s) the GPU itself produced, and the distance of the
GPU's output from it is counted in fp32 ulps at the size of the terms the element is the sum of (M = sum |w| |x| + |b| (+ |residual|) of the
launch's last conv, `f16_replay.magnitude`).  The scale of the criteria is a CPU twin per precision (below); tests/test_cpu_plan_replay.py
measures it, tests/test_gpu_plan_replay.py holds the device to 3 x the twin's figure and never to more than the a-priori bound (`cap`).

THE LAUNCH TABLE (`launch_table`), from yf_engine.hip build_plan and the launchers:

  fusion 0    one launch per layer (Builder::unit): conv0 and conv1_9 on dense3x3s2 (`l.dense`), depthwise on launch_dw (`l.dw`), every
              1x1 conv, the deconv and the two head convs on launch_pw (`l.pw`, `l.dc`, `l.head`): the fp32 VALU kernels of
              yf_conv_kernels.hip.  yf_create_ex packs MFMA fragments for plans 1 and 2 only (`for (int lvl = 1; lvl <= 2; ++lvl)`), so
              plan 0 never reaches launch_pw_mfma, and it hands every op the STORAGE dtype (`o.kdt = e->sdt()`): DT_F32 in an f16x3 engine.
  fusion 1/2  the ops of the fp16 table (build_plan does not depend on the dtype: mres_has_kernel ignores its dtype argument), on other
              kernels and in other forms:
    valu[.stem] fused_block_kernel<float>: the stem (conv0 in front), res1_1, res2_1, res2_2.  DT_F32 in every engine (launch_fused_block has
                no x3 form).
    k19r        f32 engine: k19r_kernel<8, false> (items <= 64 #CU) or <16, true>.
    k19m        f16x3 engine: k19m_kernel, NOT k19r_kernel (launch_k19m: "DT_F16X3: the region-buffer kernel").  conv1_8 is an exact fp32
                MFMA; its result is split once; conv1_9 and conv2_1 issue three products each.
    mres        mres_kernel / mres_pc_kernel<float | x3_t>, one block.  Few frames (`mres_small_batch`: 2 N tiles <= #CU): res3_3..6 on
                8x10 tiles, the conv3_5 and conv4_2 triples on 8x4 output tiles.
    mres.wexp   conv4_2+conv4_3+conv5_1, conv4_2 written as well.
    mres.chain  res4_1..4 / res5_1..5 as one launch, one dispatch.
    mres.unchained   the res4 chain at few frames: launch_chain_unchained, nblk dispatches on 8x10 tiles through the unnamed scratch tensor
                (not probe-able: the op is replayed as one unit).  f32 and f16x3.
    mres.esplit[.post]   the res5 chain at 8x10 with N <= ESPLIT_MAX_FRAMES, f32 engine only (mres_esplit_ok: `dtype == DT_F32`): nblk + 1
                dispatches of mres_esplit_kernel; at fusion 2 conv5_2 rides in the last one.
    mres[.chain].post    fusion 2: conv5_2 on the last res5 block's result in LDS, fp32 MFMAs in every engine (mres_post_conv).
    pw          fusion 1: conv5_2, deconv5_1, conv4_1_1.  All three shapes are in YF_WS_SHAPES, so launch_pw_mfma sends them to
                pw_ws_kernel / pw_ws_x3_kernel (`dtype != DT_F16`); pw_mfma_kernel<float> is not reached by any plan of the shipped shapes.
    dcat        fusion 2: dcat_kernel / dcat_x3_kernel, <1> at few frames (2 N ceil(hw / 80) <= #CU), else <DC_MT>.
    mdw, mdw.head   mdw_kernel<float | x3_t>; the stride-16 pair on 8x10 tiles at few frames.
    mdw2        fusion 2, frames that fit one 8x10 tile.
    mdw2.esplit f32 engine, 8x10 exactly, N <= MDW2_ESPLIT_MAX_FRAMES: three dispatches of mdw2_esplit_kernel.

THE TWINS.  `f32`: the launch in torch float32 on the CPU.  `f16x3`: what the x3 kernels were found to issue, which is the same in all of them
(mres_kernel, mres_pc_kernel, mdw_kernel, mdw2_kernel, pw_ws_x3_kernel, dcat_x3_kernel, k19m_kernel):
  * the activation operand of a pointwise / dense GEMM is split where it is produced: hi = rne16(a), lo = rne16(a - hi), a - hi exact in
    fp32 (yf_kernels.h split_f16x4); the weights on the host: hi = f32_to_f16_bits(w), lo = f16_lo_bits(w) -- the same two roundings;
  * THREE products per k-block, w_lo a_hi + w_hi a_lo + w_hi a_hi, accumulated in fp32 in that order; lo lo is never issued;
  * bias (and residual) are added in fp32 after the GEMM; depthwise convs, the stem / res1 / res2 blocks and conv5_2 inside the res5 launch
    are fp32 arithmetic on fp32 values (the f32 twin);
  * fp16 subnormal operands are KEPT by the MFMA (tools/mfma16_probe.hip; DESIGN_HISTORY.md): lo is subnormal for every operand below 1/8,
    so the twin rounds with gradual underflow (torch's float -> half) and flushes nothing.
"""
import dataclasses
from typing import Dict, List, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle import backbone_oracle as bo
from tests import f16_replay as fr
from tests.f16_replay import LAYER, Launch, Net, _dw64, compare, frames_u8, magnitude, state_dicts  # noqa: F401  (shared pieces, re-exported)

PRECISIONS = ("f32", "f16x3")
DT = {"f32": 0, "f16": 1, "f16x3": 2}
MARGIN = 3.0                     # the f16 replay's: the device's summation tree is a third association of the same sums
ESPLIT_MAX_FRAMES = 9            # yf_mres_kernels.hip, yf_mdw_kernels.hip (MDW2_ESPLIT_MAX_FRAMES)
REPLAY_THREADS = 16              # the CPUs a test run may use, not os.cpu_count()


# ---- one conv in the three modes -------------------------------------------------------------------------------------------------------

def split16(t):
    """hi = rne16(t), lo = rne16(t - hi), as float32 (split_f16x4; gradual underflow, nothing flushed)."""
    hi = t.half().float()
    return hi, (t - hi).half().float()


def _lin(name, x, w, b=None):
    """The linear part of layer `name` (no ReLU) in x's dtype."""
    _, kind, cin, cout, k, s, relu = LAYER[name]
    if kind == "dc":
        return F.conv_transpose2d(x, w, b, stride=2)
    if kind == "dw" and x.dtype == torch.float64:
        return _dw64(x, w, b if b is not None else torch.zeros(cout, dtype=x.dtype), k, s)
    return F.conv2d(x, w, b, stride=s if kind != "head" else 1, padding=(k - 1) // 2, groups=(x.shape[1] if kind == "dw" else 1))


class Ctx:
    """mode: 'exact' (float64), 'f32' or 'f16x3' (the twins, float32 tensors)."""

    def __init__(self, net, mode, bound=False):
        self.net, self.mode = net, mode
        self.dtype = torch.float64 if mode == "exact" else torch.float32
        self.perturb = net.perturb if mode != "exact" else {}
        self.B = {} if (bound and mode == "exact") else None   # id(tensor) -> (tensor, its propagated a-priori error bound), see `cap`

    def scale(self, *fns):
        if self.mode == "exact":
            self.net.scale = tuple(f() for f in fns if f is not None)

    def conv(self, name, x, x3=False, res=None):
        """Layer `name` (+ residual) (+ ReLU).  x3: a split-operand GEMM in an f16x3 engine."""
        _, kind, cin, cout, k, s, relu = LAYER[name]
        w, b = self.net.w(self.dtype, name, False)
        p = self.perturb
        if p.get("bias16") == name:                                    # planted: the bias rounded to fp16 before it is added
            b = b.half().to(b.dtype)
        if kind == "dw":
            y = self._dw(name, x, w, b)
        elif x3 and self.mode == "f16x3":
            (wh, wl), (xh, xl) = split16(w), split16(x)
            if p.get("flush_lo") == name:                              # planted: lo = 0 for operands below the smallest normal fp16
                wl = torch.where(w.abs() < 2.0 ** -14, torch.zeros_like(wl), wl)
                xl = torch.where(x.abs() < 2.0 ** -14, torch.zeros_like(xl), xl)
            if p.get("flush_subnormal_lo") == name:                    # planted: a lo half that is an fp16 subnormal taken as 0 (an MFMA that flushed)
                wl = torch.where(wl.abs() < 2.0 ** -14, torch.zeros_like(wl), wl)
                xl = torch.where(xl.abs() < 2.0 ** -14, torch.zeros_like(xl), xl)
            y = _lin(name, xl, wh) + _lin(name, xh, wh)
            if p.get("no_lo_hi") != name:                              # planted: w_lo a_hi left out
                y = _lin(name, xh, wl) + y
            y = y + b.view(1, -1, 1, 1)
        else:
            y = _lin(name, x, w, b)
        if res is not None:
            y = y + res
        y = F.relu(y) if relu else y
        if self.B is not None:                                         # |dy| <= |w| |dx| (+ |dres|) + terms x ulp32(M); ReLU is 1-Lipschitz
            assert not x3
            by = torch.from_numpy(ulp32(magnitude(self.net, name, x, res=res).numpy())) * _terms([name], (), (name,) if res is not None else ())
            if id(x) in self.B:
                by = by + _lin(name, self.B[id(x)][1], w.abs())
            if res is not None and id(res) in self.B:
                by = by + self.B[id(res)][1]
            self.B[id(y)] = (y, by)
        return y

    def _dw(self, name, x, w, b):
        y = _lin(name, x, w, b)
        if self.mode == "exact":
            return y
        old, self.net.perturb = self.net.perturb, {k: v for k, v in self.perturb.items() if k in ("drop_tap", "halo_frame")}
        try:                                                           # the f16 replay's two planted defects, its code
            if any(v["layer"] == name for v in self.net.perturb.values()):
                y = fr._dw_perturbed(self.net, name, x, None)          # (its conv() has applied the ReLU; the caller's is idempotent)
        finally:
            self.net.perturb = old
        p = self.perturb.get("tap_scale")
        if p and p["layer"] == name:                                   # planted: one tap's weight off by `rel`, on the last output column only
            w2 = w.clone()
            w2[:, 0, p["ky"], p["kx"]] *= 1.0 + p["rel"]
            y = y.clone()
            y[..., -1] = _lin(name, x, w2, b)[..., -1]
        return y


# ---- the launch kinds: fn(ctx, ins) -> outputs -----------------------------------------------------------------------------------------

def k_layer(name, res, x3=False):
    def fn(c, ins):
        if res:
            x, r = ins[0], ins[-1]
        else:
            x, r = (ins[0] if len(ins) == 1 else torch.cat(ins, 1)), None
        c.scale(lambda: magnitude(c.net, name, x, res=r))
        return (c.conv(name, x, x3=x3, res=r),)
    return fn


def k_valu(layers, res):
    def fn(c, ins):
        (x,) = ins
        y = x
        for n in layers[:-1]:
            y = c.conv(n, y)
        c.scale(lambda: magnitude(c.net, layers[-1], y, res=x if res else None))
        out = c.conv(layers[-1], y, res=x if res else None)
        if c.B is not None:
            c.net.bound = (c.B[id(out)][1],)
        return (out,)
    return fn


def k_k19(x3):
    def fn(c, ins):
        (x,) = ins
        y = c.conv("conv1_8", x)                    # K = 4: fp32 VALU (k19r) / one exact fp32 MFMA k-step (k19m)
        y = c.conv("conv1_9", y, x3=x3)
        c.scale(lambda: magnitude(c.net, "conv2_1", y))
        return (c.conv("conv2_1", y, x3=x3),)
    return fn


def k_mres(blocks, res, post=None, wexp=False, x3=True):
    def fn(c, ins):
        (x,) = ins
        e = None
        for bi, (a, b, p) in enumerate(blocks):
            e = c.conv(a, x, x3=x3)
            d = c.conv(b, e)
            if bi == len(blocks) - 1:
                xin = x
                c.scale(lambda: magnitude(c.net, p, d, res=xin if res else None), (lambda: magnitude(c.net, a, xin)) if wexp else None)
            x = c.conv(p, d, x3=x3, res=x if res else None)
        if post:
            xl = x
            c.scale(lambda: magnitude(c.net, post, xl))
            x = c.conv(post, x)                       # fp32 MFMAs on fp32 weights in every engine
        return (x, e) if wexp else (x,)
    return fn


def k_dcat(x3):
    def fn(c, ins):
        c52, c42 = ins
        d = c.conv("deconv5_1", c52, x3=x3)
        cat = torch.cat((c42, d), 1)
        c.scale(lambda: magnitude(c.net, "conv4_1_1", cat))
        return (c.conv("conv4_1_1", cat, x3=x3),)
    return fn


def k_mdw(pairs, head, x3):
    def fn(c, ins):
        (x,) = ins
        for i, (d, p) in enumerate(pairs):
            y = c.conv(d, x)
            if i == len(pairs) - 1 and not head:
                c.scale(lambda: magnitude(c.net, p, y))
            x = c.conv(p, y, x3=x3)
        if head:
            xl = x
            c.scale(lambda: magnitude(c.net, head, xl))
            x = c.conv(head, x, x3=x3)
        return (x,)
    return fn


# ---- the table ---------------------------------------------------------------------------------------------------------------------------

@dataclasses.dataclass
class PLaunch(Launch):
    dtype: int = 0                # what yf_op_dtype reports: the dtype the op's kernel is handed
    dispatches: int = 1           # what yf_op_dispatches reports at this batch
    form: str = ""                # the launcher's choice at this batch and CU count, restated
    terms: float = 0.0            # the a-priori forward-error bound of the launch in fp32 ulps at the terms' size (see `cap`)


def small_batch(N, H, W, th, tw, n_cu):
    """mres_small_batch and its likes: the larger tiling would leave more than half of the CUs idle."""
    return 2 * N * (-(-H // th)) * (-(-W // tw)) <= n_cu


def _terms(layers, x3_layers, res_layers=()):
    """Sum over the launch's layers of the number of terms an output sums (taps x input channels + bias (+ residual)); four times that for a
    split-operand GEMM: 22 kept operand bits against 24."""
    t = 0.0
    for n in layers:
        _, kind, cin, cout, k, s, relu = LAYER[n]
        n_terms = (k * k if kind == "dw" else cin if kind in ("dc", "head") else cin * k * k) + 1 + (1 if n in res_layers else 0)
        t += n_terms * (4.0 if n in x3_layers else 1.0)
    return t


def _res(n):
    return (n + ".conv1", n + ".conv2", n + ".conv3")


def _is_gemm(n):
    return LAYER[n][1] != "dw"


def launch_table(H, W, fusion, precision, N=2, n_cu=256, split_sums=True) -> List[PLaunch]:
    """The launches of the fp32-storage plan of an `f32` or `f16x3` engine for N frames of H x W on a device with n_cu compute units, in
    issue order (shipped io_params shape: one input channel, 24 head channels)."""
    assert precision in PRECISIONS and fusion in (0, 1, 2) and H % 32 == 0 and W % 32 == 0
    X3 = precision == "f16x3"
    kd = DT["f16x3"] if X3 else DT["f32"]
    T: List[PLaunch] = []

    def add(kind, layers, ins, outs, fn, internal=(), tiles=(), dtype=kd, dispatches=1, form="", x3_layers=None, res_layers=()):
        if x3_layers is None:
            x3_layers = [n for n in layers if _is_gemm(n)] if (X3 and dtype == DT["f16x3"]) else []
        T.append(PLaunch("+".join(layers), kind, tuple(ins), tuple(outs), tuple(internal), tuple(tiles), fn, dtype, dispatches, form,
                         _terms(layers, x3_layers, res_layers)))

    if fusion == 0:
        prev = "input"
        for name, kind, cin, cout, k, s, relu in list(bo.LAYERS) + [LAYER["head_5"], LAYER["head_4"]]:
            ins, out, res = [prev], name, False
            if name.endswith(".conv1"):
                blk_in = prev
            if name.endswith(".conv3"):
                ins, out, res = [prev, blk_in], name[:-6], True
            if name == "conv5_3" or name == "deconv5_1":
                ins = ["conv5_2"]
            if name == "conv4_1_1":
                ins = ["conv4_2", "deconv5_1"]
            if name == "head_5":
                ins, out = ["conv5_6"], "head_small"
            if name == "head_4":
                ins, out = ["conv4_1_5"], "head_large"
            lk = {"dw": "l.dw", "dc": "l.dc", "head": "l.head"}.get(kind, "l.pw" if k == 1 else "l.dense")
            add(lk, (name,), ins, [out], k_layer(name, res), dtype=DT["f32"], x3_layers=[], res_layers=(name,) if res else ())
            prev = out
        # build_plan issues each head conv directly behind its branch: head_5 after conv5_6, head_4 last
        h5 = T.pop([L.name for L in T].index("head_5"))
        T.insert([L.name for L in T].index("conv5_6") + 1, h5)
        return T

    deep = fusion == 2
    f32 = DT["f32"]

    def triple(kind, layers, x, res, tiles, out=None, form="", **kw):
        out = out or layers[-1]
        if kind.startswith("valu"):
            add(kind, layers, [x], [out], k_valu(layers, res), internal=fr._internal(layers, (), (out,)), tiles=tiles, dtype=f32, form=form,
                res_layers=(layers[-1],) if res else ())
        else:
            add(kind, layers, [x], [out], k_mres([tuple(layers)], res, **kw), internal=fr._internal(layers, (), (out,)), tiles=tiles, form=form,
                res_layers=(layers[-1],) if res else ())
        return out

    x = triple("valu.stem", ("conv0", "conv1_2", "conv1_3", "conv1_4"), "input", False, ((32, 32),))
    x = triple("valu", _res("res1_1"), x, True, ((32, 16),), out="res1_1")
    items = N * (H // 4) * (-(-(W // 4) // 16))
    if X3:
        add("k19m", ("conv1_8", "conv1_9", "conv2_1"), [x], ["conv2_1"], k_k19(True), internal=("conv1_8", "conv1_9"), tiles=((8, 16),),
            x3_layers=["conv1_9", "conv2_1"])
    else:
        add("k19r", ("conv1_8", "conv1_9", "conv2_1"), [x], ["conv2_1"], k_k19(False), internal=("conv1_8", "conv1_9"), tiles=((1, 16),),
            form="8 waves" if items <= 64 * n_cu else "16 waves, LDS weights")
    x = "conv2_1"
    for n in ("res2_1", "res2_2"):
        sm = small_batch(N, H // 4, W // 4, 32, 16, n_cu)
        x = triple("valu", _res(n), x, True, ((16, 16),) if sm else ((32, 16),), out=n, form="16x16" if sm else "32x16")
    x = triple("mres", ("conv2_2", "conv2_3", "conv3_1"), x, False, ((8, 10),))
    for n in ("res3_1", "res3_2"):
        x = triple("mres", _res(n), x, True, ((16, 20),), out=n)
    x = triple("mres", ("conv3_2", "conv3_3", "conv3_4"), x, False, ((16, 20),))
    for n in ("res3_3", "res3_4", "res3_5", "res3_6"):
        sm = small_batch(N, H // 8, W // 8, 16, 20, n_cu)
        x = triple("mres", _res(n), x, True, ((8, 10),) if sm else ((16, 20),), out=n, form="8x10" if sm else "16x20")
    sm = small_batch(N, H // 16, W // 16, 8, 10, n_cu)
    x = triple("mres", ("conv3_5", "conv3_6", "conv4_1"), x, False, ((8, 4),) if sm else ((8, 10),), form="8x4" if sm else "8x10")

    def chain(names, x, th, tw, stride, post=None, unchain=False, esplit=False):
        h, w = H // stride, W // stride
        chained = h <= th and w <= tw                                  # mres_can_chain
        groups = [names] if chained else [[n] for n in names]
        for g in groups:
            last = g is groups[-1]
            layers = tuple(l for n in g for l in _res(n)) + ((post,) if post and last else ())
            out = post if post and last else g[-1]
            kind, disp, tiles, form = "mres", 1, ((th, tw),), ""
            if len(g) > 1:
                if unchain and small_batch(N, h, w, 16, 20, n_cu):     # launch_mres: not DT_F16, scratch tensor, no post conv
                    kind, disp, tiles, form = "mres.unchained", len(g), ((8, 10),), "block by block on 8x10 tiles"
                elif esplit and not X3 and split_sums and (h, w) == (8, 10) and N <= ESPLIT_MAX_FRAMES:
                    kind, disp, form = "mres.esplit", len(g) + 1, "mres_esplit_kernel"
                else:
                    kind, form = "mres.chain", "one launch"
            if post and last:
                kind += ".post"
            add(kind, layers, [x], [out], k_mres([_res(n) for n in g], True, post=post if last else None), internal=fr._internal(layers, g, (out,)),
                tiles=tiles, dispatches=disp, form=form, x3_layers=[l for l in layers if _is_gemm(l) and l != post] if X3 else [],
                res_layers=tuple(n + ".conv3" for n in g))
            x = out
        return x

    x = chain(["res4_1", "res4_2", "res4_3", "res4_4"], x, 16, 20, 16, unchain=True)
    sm = small_batch(N, H // 32, W // 32, 8, 10, n_cu)
    add("mres.wexp", ("conv4_2", "conv4_3", "conv5_1"), [x], ["conv5_1", "conv4_2"], k_mres([("conv4_2", "conv4_3", "conv5_1")], False, wexp=True),
        internal=("conv4_3",), tiles=((8, 4),) if sm else ((8, 10),), form="8x4" if sm else "8x10")
    x = chain(["res5_1", "res5_2", "res5_3", "res5_4", "res5_5"], "conv5_1", 8, 10, 32, post="conv5_2" if deep else None, esplit=True)
    if not deep:
        add("pw", ("conv5_2",), [x], ["conv5_2"], k_layer("conv5_2", False, x3=True))
    h32, w32 = H // 32, W // 32
    if deep and h32 <= 8 and w32 <= 10:                                 # mdw2_can_chain
        es = not X3 and split_sums and (h32, w32) == (8, 10) and N <= ESPLIT_MAX_FRAMES
        add("mdw2.esplit" if es else "mdw2", ("conv5_3", "conv5_4", "conv5_5", "conv5_6", "head_5"), ["conv5_2"], ["head_small"],
            k_mdw([("conv5_3", "conv5_4"), ("conv5_5", "conv5_6")], "head_5", True), internal=("conv5_3", "conv5_4", "conv5_5", "conv5_6"),
            tiles=((8, 10),), dispatches=3 if es else 1, form="mdw2_esplit_kernel" if es else "one launch")
    else:
        add("mdw", ("conv5_3", "conv5_4"), ["conv5_2"], ["conv5_4"], k_mdw([("conv5_3", "conv5_4")], None, True), internal=("conv5_3",), tiles=((8, 10),))
        add("mdw.head", ("conv5_5", "conv5_6", "head_5"), ["conv5_4"], ["head_small"], k_mdw([("conv5_5", "conv5_6")], "head_5", True),
            internal=("conv5_5", "conv5_6"), tiles=((8, 10),))
    if deep:
        sm = 2 * N * (-(-(h32 * w32) // 80)) <= n_cu
        add("dcat", ("deconv5_1", "conv4_1_1"), ["conv5_2", "conv4_2"], ["conv4_1_1"], k_dcat(True), internal=("deconv5_1",),
            form="one M-tile per item" if sm else "five M-tiles per item")
    else:
        add("pw", ("deconv5_1",), ["conv5_2"], ["deconv5_1"], k_layer("deconv5_1", False, x3=True))
        add("pw", ("conv4_1_1",), ["conv4_2", "deconv5_1"], ["conv4_1_1"], k_layer("conv4_1_1", False, x3=True))
    h16 = H // 16
    sm = h16 > 8 and small_batch(N, h16, W // 16, 16, 20, n_cu)         # launch_mdw: `a.H > 8 && 2 * big_tiles <= n_cu`
    tl, fm = (((8, 10),), "8x10") if sm else (((16, 20),), "16x20")
    add("mdw", ("conv4_1_2", "conv4_1_3"), ["conv4_1_1"], ["conv4_1_3"], k_mdw([("conv4_1_2", "conv4_1_3")], None, True), internal=("conv4_1_2",),
        tiles=tl, form=fm)
    add("mdw.head", ("conv4_1_4", "conv4_1_5", "head_4"), ["conv4_1_3"], ["head_large"], k_mdw([("conv4_1_4", "conv4_1_5")], "head_4", True),
        internal=("conv4_1_4", "conv4_1_5"), tiles=tl, form=fm)
    return T


def forms(table) -> Dict[str, Tuple[str, int, str]]:
    """{op name: (kind, dispatches, form)}: what each case asserts it reaches."""
    return {L.name: (L.kind, L.dispatches, L.form) for L in table}


def forms_text(table):
    return "\n".join("  %-16s x%d  dtype %d  %-28s %s" % (L.kind, L.dispatches, L.dtype, L.form, L.name[:60]) for L in table)


# ---- running -----------------------------------------------------------------------------------------------------------------------------

def run(launch, net, inputs, mode):
    """One launch from the given input tensors in `mode` ('exact' | 'f32' | 'f16x3') -> {name: output}."""
    c = Ctx(net, mode, bound=launch.kind in PROPAGATED_CAP)
    with torch.no_grad():
        outs = launch.fn(c, tuple(inputs[n].to(c.dtype) for n in launch.inputs))
    return dict(zip(launch.outputs, outs))


def chained(table, net, x, mode):
    t = {"input": x}
    for L in table:
        t.update(run(L, net, t, mode))
    return t


# ---- the comparator ----------------------------------------------------------------------------------------------------------------------

def ulp32(m):
    """One fp32 ulp at |m| (float64 array): 2^(floor(log2 m) - 23); subnormals counted as the smallest normal's."""
    return np.exp2(np.floor(np.log2(np.maximum(np.abs(m), 2.0 ** -126))) - 23)


@dataclasses.dataclass
class Dist:
    dist: float          # largest |got - exact| in fp32 ulps at max(|exact|, M)
    own: float           # ... in the result's own fp32 ulps (results below 2^-20 counted as 2^-20): reported only
    where: str           # the worst elements and what they have in common (f16_replay.compare's text)
    cap_used: float = 0.0   # largest |got - exact| as a share of the a-priori bound (the launch's cap)


def distance(got, exact64, scale64, tiles=(), limit=None, cap_ulps=None, bound64=None) -> Dist:
    """limit, cap_ulps: in fp32 ulps at the terms' size; bound64: the propagated bound per element (absolute), which replaces cap_ulps."""
    g, e = got.detach().cpu().double(), exact64.detach().cpu().double()
    assert g.shape == e.shape, (g.shape, e.shape)
    assert bool(torch.isfinite(g).all()), "a non-finite output"
    m = np.maximum(np.abs(e.numpy()), scale64.detach().cpu().double().numpy())
    err = np.abs(g.numpy() - e.numpy())
    d = err / ulp32(m)
    out = Dist(float(d.max()), float((err / ulp32(np.maximum(np.abs(e.numpy()), 2.0 ** -20))).max()), "")
    if bound64 is not None:                     # per element: min(limit ulps, bound); expressed as a distance scaled so that `limit` is the criterion
        b = bound64.numpy() / ulp32(m)
        out.cap_used = float((d / b).max())
        if limit is not None:
            d = d * (limit / np.minimum(limit, b))
    elif cap_ulps:
        out.cap_used = out.dist / cap_ulps
    if limit is not None and float(d.max()) > limit:
        # the location report of the f16 comparator, handed the distances themselves (scaled so that its fp32 criterion, 2e-5, is the limit)
        c = compare(torch.from_numpy(d * (2e-5 / limit)), torch.zeros(e.shape, dtype=torch.float64), None, tiles, fp32=True)
        i = np.unravel_index(int(d.argmax()), d.shape)
        out.where = "%s; worst (n=%d, c=%d, y=%d, x=%d): got %.9g, exact %.9g, terms' size %.3g" % (
            c.where.split("; worst:")[0], *i, float(g[i]), float(e[i]), float(m[i]))
    return out


# THE CAP.  A launch's limit may not exceed its a-priori forward-error bound: the sum, over the launch's layers, of the number of terms an
# output sums, in fp32 ulps at the terms' size (four times that for a split-operand GEMM) -- PLaunch.terms.  The twin stays inside it in
# every kind but the fp32 VALU block launches (tests/test_cpu_plan_replay.py asserts both):
#   valu.stem  conv0+conv1_2+conv1_3+conv1_4: up to 2921 ulps from float64 where the sum is 38;
#   valu       res1_1: 24.1 where the sum is 25 over the parametrisation, and 28.5 with the shipped weights at 160x224, N = 36.
# The model is not wrong -- each of these layers, replayed alone at fusion 0, is within 7 ulps -- the sum is: it counts every layer's rounding
# at the LAST conv's terms' size, but that conv's terms can be hundreds of times smaller than those of the layers in front of it (the worst
# element of the stem: conv1_3's ReLU output is a small difference of large terms, so M of conv1_4 is 0.0018 where conv0's terms are of order
# 1), and their roundings arrive at full size.  These stride-2 blocks are where the net is worst conditioned; from stride 4 on the twin uses
# at most a tenth of the sum.  For the kinds named here the cap is therefore the same bound PROPAGATED: per element, |dy| <= sum |w| |dx|
# (+ |d residual|) + terms x ulp32(M of this layer), layer by layer from a zero input error (running error analysis; ReLU is 1-Lipschitz).
# For a single layer it IS the sum above.  Still a condition, not a measurement.
PROPAGATED_CAP = ("valu.stem", "valu")


def cap(launch):
    """The a-priori forward-error bound of a launch in fp32 ulps at the terms' size (kinds in PROPAGATED_CAP: per element, from the replay)."""
    return launch.terms


def limit(precision, launch, reference=None):
    """The GPU criterion of a launch: the margin times the twin's worst distance of its (precision, kind), never more than the cap."""
    ref = (reference or REFERENCE)[(precision, launch.kind)]
    return MARGIN * ref if launch.kind in PROPAGATED_CAP else min(MARGIN * ref, cap(launch))


def replay_and_check(launch, net, tensors, got, precision=None, reference=None):
    """The float64 replay of one launch from `tensors` against `got` -> [(out_name, Dist, verdict or None)]."""
    net.scale = net.bound = None
    exact = run(launch, net, tensors, "exact")
    lim = limit(precision, launch, reference) if precision else None
    prop = launch.kind in PROPAGATED_CAP
    res = []
    for i, ((name, e), m) in enumerate(zip(exact.items(), net.scale)):
        d = distance(got[name], e, m, launch.tiles, lim, cap(launch), net.bound[i] if prop else None)
        v = None
        if d.where:
            v = ("launch %s [%s, %s, %d dispatch(es), %s] -> %s: largest distance %.2f fp32 ulps at the terms' size (limit %.2f = 3 x twin, cap %s, of "
                 "which %.2f are used; %.0f in the result's own ulps); %s" % (
                     launch.name, launch.kind, precision, launch.dispatches, launch.form or "-", name, d.dist, lim,
                     "propagated per element" if prop else "%.0f" % cap(launch), d.cap_used, d.own, d.where))
        res.append((name, d, v))
    return res


def heads_rule(got_l, got_s, ref32, ref64, ratio=3.0, floor=5e-5):
    """tests/test_gpu_parity.py _check_heads' arithmetic: max |got - ref64| <= max(3 x max |torch fp32 - ref64|, 5e-5) at both heads."""
    ok = True
    for got, r32, r64 in ((got_l, ref32[0], ref64[0]), (got_s, ref32[1], ref64[1])):
        ours = float((got.double() - r64.double()).abs().max())
        theirs = float((r32.double() - r64.double()).abs().max())
        ok &= ours <= max(ratio * theirs, floor)
    return ok


class Net64(Net):
    """The BatchNorm fold in float64 WITHOUT the rounding to fp32: what the float64 launches must chain to the reference's graph with."""

    def __init__(self, sd):
        from oracle.fp16_rounding_sim import fold
        sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
        self.f32 = {}
        for name, kind, cin, cout, k, s, relu in bo.LAYERS:
            w = sd64[name + ".0.weight"]
            sc = sd64[name + ".1.weight"] / torch.sqrt(sd64[name + ".1.running_var"] + bo.BN_EPS)
            self.f32[name] = (w * (sc[None, :, None, None] if kind == "dc" else sc[:, None, None, None]), sd64[name + ".1.bias"] - sd64[name + ".1.running_mean"] * sc)
        for h in ("head_5", "head_4"):
            self.f32[h] = (sd64[h + ".weight"], sd64[h + ".bias"])
        assert set(self.f32) == set(fold(sd))
        self._cache, self.perturb = {}, {}


# ---- cases -------------------------------------------------------------------------------------------------------------------------------

# (H, W, N, fusion levels, precisions): tests/test_gpu_plan_replay.py's parametrisation; what each reaches is asserted by `expect`
CASES = (
    (96, 160, 2, (1, 2), PRECISIONS),
    (96, 160, 132, (1, 2), PRECISIONS),
    (160, 224, 2, (1, 2), PRECISIONS),
    (160, 224, 36, (1, 2), PRECISIONS),
    (256, 352, 2, (1, 2), PRECISIONS),
    (256, 320, 2, (1, 2), ("f32",)),
    (256, 320, ESPLIT_MAX_FRAMES, (1, 2), ("f32",)),
    (256, 320, ESPLIT_MAX_FRAMES + 1, (1, 2), ("f32",)),
    (96, 160, 2, (0,), PRECISIONS),
    (160, 224, 36, (0,), PRECISIONS),
)
RANDOM_ONLY = {(96, 160, 132), (160, 224, 36)}        # the large batches run with the seeded random weights only (a few seconds per test)

RES4 = "+".join(l for n in ("res4_1", "res4_2", "res4_3", "res4_4") for l in _res(n))
RES5 = "+".join(l for n in ("res5_1", "res5_2", "res5_3", "res5_4", "res5_5") for l in _res(n))
MDW2 = "conv5_3+conv5_4+conv5_5+conv5_6+head_5"


def expect(H, W, N, fusion, precision, n_cu):
    """{op name: (kind, dispatches)} a case exists for, for a device of n_cu compute units (256 on an MI355X)."""
    if fusion == 0:
        return {}
    post = "+conv5_2" if fusion == 2 else ""
    p = ".post" if fusion == 2 else ""
    few = {(96, 160): 2 * N <= n_cu, (160, 224): 2 * N <= n_cu, (256, 320): 2 * N <= n_cu}.get((H, W))
    e = {}
    if (H, W) in ((96, 160), (160, 224)):
        e[RES4] = ("mres.unchained", 4) if few else ("mres.chain", 1)
        e[RES5 + post] = ("mres.chain" + p, 1)
        if fusion == 2:
            e[MDW2] = ("mdw2", 1)
    if (H, W) == (256, 352):
        for n in ("res4_1", "res5_1"):
            e["+".join(_res(n))] = ("mres", 1)
        e["conv5_3+conv5_4"] = ("mdw", 1)
        e["conv5_5+conv5_6+head_5"] = ("mdw.head", 1)
    if (H, W) == (256, 320):
        es = precision == "f32" and N <= ESPLIT_MAX_FRAMES
        e[RES4] = ("mres.unchained", 4) if few else ("mres.chain", 1)
        e[RES5 + post] = ("mres.esplit" + p, 6) if es else ("mres.chain" + p, 1)
        if fusion == 2:
            e[MDW2] = ("mdw2.esplit", 3) if es else ("mdw2", 1)
    return e


# The twin's worst distance from the float64 replay per (precision, launch kind), in fp32 ulps at the terms' size, over the whole
# parametrisation (CASES x weights): tests/test_cpu_plan_replay.py measures them again and asserts that none is exceeded; the GPU is held to
# MARGIN times these, and never to more than a launch's cap.
REFERENCE: Dict[Tuple[str, str], float] = {
    ('f16x3', 'dcat'): 5.34,
    ('f16x3', 'k19m'): 13.39,
    ('f16x3', 'l.dc'): 3.82,
    ('f16x3', 'l.dense'): 3.42,
    ('f16x3', 'l.dw'): 4.34,
    ('f16x3', 'l.head'): 5.72,
    ('f16x3', 'l.pw'): 7.10,
    ('f16x3', 'mdw'): 7.52,
    ('f16x3', 'mdw.head'): 6.29,
    ('f16x3', 'mdw2'): 4.61,
    ('f16x3', 'mres'): 8.50,
    ('f16x3', 'mres.chain'): 14.10,
    ('f16x3', 'mres.chain.post'): 5.95,
    ('f16x3', 'mres.post'): 3.30,
    ('f16x3', 'mres.unchained'): 12.89,
    ('f16x3', 'mres.wexp'): 7.88,
    ('f16x3', 'pw'): 7.49,
    ('f16x3', 'valu'): 12.41,
    ('f16x3', 'valu.stem'): 2979.31,
    ('f32', 'dcat'): 5.86,
    ('f32', 'k19r'): 4.91,
    ('f32', 'l.dc'): 3.82,
    ('f32', 'l.dense'): 3.42,
    ('f32', 'l.dw'): 4.34,
    ('f32', 'l.head'): 5.72,
    ('f32', 'l.pw'): 7.10,
    ('f32', 'mdw'): 5.97,
    ('f32', 'mdw.head'): 5.90,
    ('f32', 'mdw2'): 5.60,
    ('f32', 'mdw2.esplit'): 5.41,
    ('f32', 'mres'): 6.26,
    ('f32', 'mres.chain'): 11.97,
    ('f32', 'mres.chain.post'): 4.75,
    ('f32', 'mres.esplit'): 8.66,
    ('f32', 'mres.esplit.post'): 4.75,
    ('f32', 'mres.post'): 3.48,
    ('f32', 'mres.unchained'): 10.09,
    ('f32', 'mres.wexp'): 4.59,
    ('f32', 'pw'): 5.88,
    ('f32', 'valu'): 24.60,
    ('f32', 'valu.stem'): 2979.31,
}
