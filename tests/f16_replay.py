"""TEST INFRASTRUCTURE (CPU only, never imported by the product): the fp16-storage plan (`dtype f16`) replayed ONE LAUNCH AT A TIME against
a model that rounds where the kernel rounds.

The head-level fp16 bounds of tests/test_gpu_parity.py are 2 .. 4 fp16 ulps at the heads and hundreds of ulps at an interior tensor, because
86 layers of legitimate rounding have accumulated there.  Here the accumulation is removed: every launch of the plan is evaluated in float64
from the input tensor(s) the GPU itself produced (fp16 values, exactly representable), with round-to-nearest-even to fp16 at exactly the
places where that launch rounds, and the GPU's output is compared with it element by element.  The same launch functions run on float32
tensors (the "twin", torch CPU): twin against float64 is the reference's own noise and sets the scale of the GPU criteria
(tests/test_cpu_f16_replay.py), and the twin chained over the whole net is bitwise `oracle.fp16_rounding_sim.Sim(W, T, A, E, size, fusion)`.

WEIGHTS.  `packer.pack_state_dict` folds BatchNorm in float64 (`fold_bn`) and rounds ONCE to fp32; the engine packs fp16 fragments from those
fp32 values with `f32_to_f16_bits` (RNE; yf_mfma_kernels.hip).  `Net` unpacks the blob the engine is given, so the fp32 values are the GPU's.
Biases and depthwise weights stay fp32 in every kernel ("b1 / wd / bd / b2 stay fp32", yf_mres_kernels.hip mres_pack_weights).

ROUNDING POINTS PER LAUNCH KIND (W = weights of an MFMA layer rounded, A = activation operand of a pointwise MFMA rounded, T = tensor
written to HBM rounded; everything else is fp32 arithmetic on fp32 values, modelled in float64):

  valu        fused_block_kernel<.., half_t> (yf_fused_kernels.hip): the stem (conv0 from the fp32 input planes) and res1_1, res2_1, res2_2.
              fp32 weights through the scalar path, E in LDS as float (`__shared__ float E[]`), packed fp32 FMAs.  ONE rounding: the store
              `st4<T>(o + co, v)` after bias (+ residual `ld4<T>`) -- T.
  k19h        k19h_kernel (yf_k19_kernels.hip): conv1_8 W `(half_t)a.w8[..]`, bias = the MFMA's C operand, result RNE + ReLU
              (`__builtin_elementwise_max(__builtin_convertvector(d0, f16x4), zero4)`) -- the one E rounding of the plan --; conv1_9 W
              (k19h_pack_weights), `acc0 + bias9a` RNE + ReLU = conv2_1's operand (A); conv2_1 W, bias21 as C, `__builtin_convertvector(o, f16x4)`
              store (T).
  mres        mres_kernel / mres_pc_kernel<.., half_t> (yf_mres_kernels.hip): X tile in LDS as float (the fp16 input, exact); expansion W
              (mres_pack_weights `f32_to_f16_bits`), A `(half_t)a1[i][..]`, bias b1 as C, ReLU -> E in LDS as FLOAT
              (`*reinterpret_cast<float4*>(E + ..) = ev`: NOT rounded); depthwise fp32 weights + bias, `(half_t)fmaxf(d[0], 0.f)` = the
              projection's operand (A); projection W; epilogue `acc + bias (+ x from X)` [ReLU for conv5_1], `st4<T>` (T).
  mres.wexp   conv4_2+conv4_3+conv5_1: the same, and `st4<T>(a.out_exp .., ev)` writes conv4_2 rounded (T) while conv4_3 reads the
              un-rounded E.
  mres.chain  res4_1..4 / res5_1..5 as one launch (mres_pc_kernel, MresArgs::nblk; frames that fit one tile): a block's result replaces X
              in LDS as FLOAT (`*reinterpret_cast<float4*>(xr) = v`): between blocks NO T; the next expansion rounds its operand (A) and
              the residual adds the un-rounded value; only the last block stores (T).
  mres.post   fusion 2: + conv5_2 on the last res5 block's un-rounded result in LDS, fp32 MFMAs on fp32 weights (mres_post_conv:
              `__builtin_amdgcn_mfma_f32_16x16x4f32`, no W, no A), bias, ReLU, `st4<T>` (T).  res5_5 itself never exists in memory.
  pw          pw_mfma_kernel<.., half_t> (yf_mfma_kernels.hip): conv5_2 / deconv5_1 / conv4_1_1 at fusion 1.  Operand as it lies in HBM,
              W (mfma_pack_weights_f16), acc + bias, ReLU, `st4<T>` (T).
  dcat        dcat_h_kernel (yf_dcat_kernels.hip), fusion 2: deconv W, `__builtin_convertvector(dacc[nt] + b, f16x4)` + ReLU in registers
              (= the T rounding of the deconv launch it replaces); conv4_1_1 W; `__builtin_convertvector(cacc[nt] + b, f16x4)` store (T).
  mdw         mdw_kernel<.., half_t> (yf_mdw_kernels.hip): depthwise 5x5 fp32, `(half_t)fmaxf(d2.., 0.f)` (A); 1x1 conv W; + bias; `st4<TT>` (T).
  mdw.head    the same with the head conv chained: `(half_t)hv[..]` (A), head W, `h[nth][reg] + hb[hc]` stored as fp32 NCHW: no rounding.
  mdw2        mdw2_kernel, fusion 2, frames that fit one 8x10 tile: stage 1's result `+ bias -> Y` in LDS as float: conv5_4 NOT rounded;
              stage 2 as mdw.head.

FUSION 0 has no fp16-storage form: run_forward refuses it ("fp16 storage needs a fused plan", yf_engine.hip); the table covers levels 1 and 2.
The few-frames split-sum launches and launch_mres's block-by-block form are fp32-only (`dtype != DT_F16`, `dtype == DT_F32`): with fp16
storage a batch size only selects tile shapes (`mres_small_batch`: 2 N tiles <= #CU).
"""
import dataclasses
from typing import Callable, Dict, List, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle import backbone_oracle as bo

LAYER = dict(bo._BY_NAME)
for _h, _cin in (("head_5", 128), ("head_4", 96)):
    LAYER[_h] = (_h, "head", _cin, 24, 1, 1, False)

# what the GPU criteria are multiples of: test_cpu_f16_replay.py measures the float32 twin against the float64 replay per launch kind over
# the whole parametrisation and asserts that nothing exceeds these (share of elements that differ, largest distance in fp16 ulps)
SHARE_CAP, ULP_CAP = 0.02, 8.0
MARGIN = 3.0                       # the GPU's summation tree is a third association of the same sums
F32_RTOL = 2e-5                    # fp32 outputs (the heads): test_layer_probes_match_reference's criterion for one launch


def rne16(t):
    """Round to nearest even to fp16, dtype kept.  float64 goes through numpy: torch's double -> half converts through float (double rounding)."""
    if t.dtype == torch.float64:
        return torch.from_numpy(t.numpy().astype(np.float16).astype(np.float64))
    return t.half().to(t.dtype)


class Net:
    """The folded fp32 weights the engine is given (packer blob), as conv weights in any dtype, plain and rounded to fp16."""

    def __init__(self, sd, num_out=24, input_channel=1):
        from yolo_fastest_amd import packer
        lay = packer.unpack(packer.pack_state_dict({k: v.detach().cpu() for k, v in sd.items()}, num_out, input_channel))
        self.f32 = {}
        for name, d in lay.items():
            cin, cout, k = d["cin"], d["cout"], d["k"]
            w = torch.from_numpy(np.array(d["w"]))
            kind = LAYER[name][1]
            if kind == "dw":
                w = w.view(k, k, cout).permute(2, 0, 1)[:, None]
            elif kind == "dc":
                w = w.view(2, 2, cin, cout).permute(2, 3, 0, 1)
            elif k == 1:
                w = w.view(cin, cout).t()[:, :, None, None]
            else:
                w = w.view(k, k, cin, cout).permute(3, 2, 0, 1)
            self.f32[name] = (w.contiguous(), torch.from_numpy(np.array(d["b"])))
        self._cache = {}
        self.perturb = {}    # test_cpu_f16_replay.py: deliberate mistakes of the float32 twin, keyed by kind

    def w(self, dtype, name, rounded):
        key = (dtype, name, rounded)
        if key not in self._cache:
            w, b = self.f32[name]
            self._cache[key] = ((rne16(w) if rounded else w).to(dtype), b.to(dtype))
        return self._cache[key]


def _dw64(x, w, b, k, s):
    """Depthwise conv as shifted multiply-adds (torch's float64 grouped conv is a slow generic path)."""
    p = (k - 1) // 2
    xp = F.pad(x, (p, p, p, p))
    Ho, Wo = (x.shape[2] + 2 * p - k) // s + 1, (x.shape[3] + 2 * p - k) // s + 1
    y = b.view(1, -1, 1, 1).expand(x.shape[0], -1, Ho, Wo).clone()
    for ky in range(k):
        for kx in range(k):
            y += xp[:, :, ky:ky + (Ho - 1) * s + 1:s, kx:kx + (Wo - 1) * s + 1:s] * w[:, 0, ky, kx].view(1, -1, 1, 1)
    return y


def magnitude(net, name, x, W=False, res=None):
    """sum |w| |x| + |b| (+ |residual|) of the conv `name`: the size of the terms whose sum an output element is, i.e. what an fp32
    evaluation of it rounds at (float64)."""
    _, kind, cin, cout, k, s, relu = LAYER[name]
    w, b = net.w(torch.float64, name, W)
    x = x.double().abs()
    if kind == "dc":
        y = F.conv_transpose2d(x, w.abs(), b.abs(), stride=2)
    elif kind == "dw":
        y = _dw64(x, w.abs(), b.abs(), k, s)
    else:
        y = F.conv2d(x, w.abs(), b.abs(), stride=s, padding=(k - 1) // 2)
    return y if res is None else y + res.double().abs()


def conv(net, name, x, W=False, bias=True, w_override=None):
    """One folded conv (+ ReLU) of the layer table in x's dtype: oracle/fp16_rounding_sim.py Sim.unit's calls, so that the float32 twin is
    bitwise Sim.  W: the fp16-rounded weights."""
    _, kind, cin, cout, k, s, relu = LAYER[name]
    w, b = net.w(x.dtype, name, W)
    if w_override is not None:
        w = w_override
    if not bias:
        b = None
    if kind == "dc":
        y = F.conv_transpose2d(x, w, b, stride=2)
    elif kind == "head":
        y = F.conv2d(x, w, b)
    elif kind == "dw" and x.dtype == torch.float64:
        y = _dw64(x, w, b if b is not None else torch.zeros(cout, dtype=x.dtype), k, s)
    else:
        y = F.conv2d(x, w, b, stride=s, padding=(k - 1) // 2, groups=(x.shape[1] if kind == "dw" else 1))
    return F.relu(y) if relu else y


def _scale(net, like, *fns):
    """Record the magnitude of the launch's final sum(s), one per output, while the float64 replay runs."""
    if like.dtype == torch.float64:
        net.scale = tuple(f() for f in fns if f is not None)


# ---- the launch kinds ----------------------------------------------------------------------------------------------------------------

def _mistake(net, like, key):
    """The float32 twin's deliberate mistake `key`, if one is asked for; the float64 replay never makes any."""
    return net.perturb.get(key) if like.dtype == torch.float32 else None


def _dw_perturbed(net, name, e, launch):
    """The depthwise layer `name`, with the twin's deliberate mistakes where asked for."""
    y = conv(net, name, e)
    p = _mistake(net, e, "drop_tap")
    if p and p["layer"] == name:                       # one tap omitted on the last output column only
        w = net.w(e.dtype, name, False)[0].clone()
        w[:, 0, p["ky"], p["kx"]] = 0
        y = y.clone()
        y[..., -1] = conv(net, name, e, w_override=w)[..., -1]
    p = _mistake(net, e, "halo_frame")
    if p and p["layer"] == name:                       # the halo row below the first row of tiles: frame 1 reads frame 0's
        th = p["tile_h"]
        assert e.shape[0] >= 2 and e.shape[2] > th and LAYER[name][5] == 1
        e2 = e.clone()
        e2[1, :, th] = e[0, :, th]
        y = y.clone()
        y[1, :, th - 1] = conv(net, name, e2)[1, :, th - 1]
    return y


def k_valu(layers, res):
    def fn(net, ins):
        (x,) = ins
        if len(layers) == 4:
            x = conv(net, layers[0], x)
        a, b, c = layers[-3:]
        y = conv(net, a, x)
        y = _dw_perturbed(net, b, y, None)
        _scale(net, y, lambda: magnitude(net, c, y, res=x if res else None))
        y = conv(net, c, y)
        if res:
            y = y + x
        return (rne16(y),)
    return fn


def k_k19h():
    def fn(net, ins):
        (x,) = ins
        y = rne16(conv(net, "conv1_8", rne16(x), W=True))          # E: the one expanded tensor that is rounded
        p = _mistake(net, y, "swap_channels")
        if p:
            i, j = p["pair"]
            y = y.clone()
            y[:, [i, j]] = y[:, [j, i]]
        y = conv(net, "conv1_9", rne16(y), W=True)
        _scale(net, y, lambda: magnitude(net, "conv2_1", rne16(y), W=True))
        y = conv(net, "conv2_1", rne16(y), W=True)
        return (rne16(y),)
    return fn


def k_mres(blocks, res, post=None, wexp=False):
    """blocks: [(expand, depthwise, project), ...] -- more than one = a chained launch."""
    def fn(net, ins):
        (x,) = ins
        e = None
        for bi, (a, b, c) in enumerate(blocks):
            e = conv(net, a, rne16(x), W=True)                      # A (the launch's input is fp16 already; a chained block's is not)
            d = _dw_perturbed(net, b, e, None)
            skip_a = _mistake(net, d, "skip_a") == c
            late_bias = _mistake(net, d, "late_bias") == c and bi == len(blocks) - 1 and not post
            if bi == len(blocks) - 1:
                xin = x
                _scale(net, d, lambda: magnitude(net, c, rne16(d), W=True, res=xin if res else None),
                       (lambda: magnitude(net, a, rne16(xin), W=True)) if wexp else None)
            y = conv(net, c, d if skip_a else rne16(d), W=True, bias=not late_bias)
            if res:
                y = y + x
            if late_bias:                                            # the twin's mistake: round, THEN add the bias
                return (rne16(y) + net.w(y.dtype, c, False)[1].view(1, -1, 1, 1),)
            x = y
        if post:
            _scale(net, x, lambda: magnitude(net, post, x))
        out = rne16(conv(net, post, x)) if post else rne16(x)       # conv5_2 on the un-rounded tile, fp32 weights
        return (out, rne16(e)) if wexp else (out,)
    return fn


def k_pw(name):
    def fn(net, ins):
        x = ins[0] if len(ins) == 1 else torch.cat(ins, 1)
        _scale(net, x, lambda: magnitude(net, name, x, W=True))
        return (rne16(conv(net, name, rne16(x), W=True)),)
    return fn


def k_dcat():
    def fn(net, ins):
        c52, c42 = ins
        d = rne16(conv(net, "deconv5_1", rne16(c52), W=True))
        _scale(net, d, lambda: magnitude(net, "conv4_1_1", torch.cat((c42, d), 1), W=True))
        return (rne16(conv(net, "conv4_1_1", rne16(torch.cat((c42, d), 1)), W=True)),)
    return fn


def k_mdw(pairs, head):
    """pairs: [(depthwise, pointwise), ...] -- two = mdw2_kernel, the first pair's result stays in LDS un-rounded."""
    def fn(net, ins):
        (x,) = ins
        for i, (d, p) in enumerate(pairs):
            y = _dw_perturbed(net, d, x, None)
            if i == len(pairs) - 1 and not head:
                _scale(net, y, lambda: magnitude(net, p, rne16(y), W=True))
            x = conv(net, p, rne16(y), W=True)
        if head:
            _scale(net, x, lambda: magnitude(net, head, rne16(x), W=True))
            return (conv(net, head, rne16(x), W=True),)
        return (rne16(x),)
    return fn


@dataclasses.dataclass
class Launch:
    name: str                     # the engine's name of the op: its layers joined by '+' (yf_op_info_ex)
    kind: str
    inputs: Tuple[str, ...]       # tensors that exist in device memory (yf_forward_probe)
    outputs: Tuple[str, ...]      # ... 'head_large' / 'head_small' are the forward's results, fp32
    internal: Tuple[str, ...]     # tensors of the reference module that this launch keeps on chip: YF_E_NOPROBE, replayed as part of it
    tiles: Tuple[Tuple[int, int], ...]   # output tile shapes the launch may use (many / few frames): where a seam would show
    fn: Callable

    @property
    def fp32_out(self):
        return self.outputs[0].startswith("head_")


def _res(n):
    return (n + ".conv1", n + ".conv2", n + ".conv3")


def _internal(layers, blocks, outs):
    """Tensors of the reference module inside a launch that are not its outputs (a block's conv3 is not a tensor of its own: the engine names
    the sum after it by the block; the head convs' results are the forward's outputs)."""
    return tuple(n for n in tuple(layers) + tuple(blocks) if n not in outs and not n.endswith(".conv3") and not n.startswith("head_"))


def launch_table(H, W, fusion) -> List[Launch]:
    """The launches of the fp16-storage plan for H x W frames (yf_engine.hip build_plan, fused plans, shipped io_params shape: at most four
    input channels, a head mdw_kernel is instantiated for), in issue order."""
    if fusion not in (1, 2):
        raise ValueError("fp16 storage needs a fused plan: fusion 1 or 2 (yf_engine.hip run_forward refuses level 0)")
    assert H % 32 == 0 and W % 32 == 0
    deep = fusion == 2
    T: List[Launch] = []

    def add(kind, layers, ins, outs, fn, internal=(), tiles=()):
        T.append(Launch("+".join(layers), kind, tuple(ins), tuple(outs), tuple(internal), tuple(tiles), fn))

    def triple(kind, layers, x, res, tiles, out=None, **kw):
        out = out or layers[-1]
        fn = k_valu(layers, res) if kind == "valu" else k_mres([tuple(layers)], res, **kw)
        add(kind, layers, [x], [out], fn, internal=_internal(layers, (), (out,)), tiles=tiles)
        return out

    x = triple("valu", ("conv0", "conv1_2", "conv1_3", "conv1_4"), "input", False, ((32, 32),))
    x = triple("valu", _res("res1_1"), x, True, ((32, 16), (16, 16)), out="res1_1")
    add("k19h", ("conv1_8", "conv1_9", "conv2_1"), [x], ["conv2_1"], k_k19h(), internal=("conv1_8", "conv1_9"), tiles=((1, 16),))
    x = "conv2_1"
    for n in ("res2_1", "res2_2"):
        x = triple("valu", _res(n), x, True, ((32, 16), (16, 16)), out=n)
    x = triple("mres", ("conv2_2", "conv2_3", "conv3_1"), x, False, ((8, 10), (8, 4)))
    for n in ("res3_1", "res3_2"):
        x = triple("mres", _res(n), x, True, ((16, 20), (8, 10)), out=n)
    x = triple("mres", ("conv3_2", "conv3_3", "conv3_4"), x, False, ((16, 20), (8, 10)))
    for n in ("res3_3", "res3_4", "res3_5", "res3_6"):
        x = triple("mres", _res(n), x, True, ((16, 20), (8, 10)), out=n)
    x = triple("mres", ("conv3_5", "conv3_6", "conv4_1"), x, False, ((8, 10), (8, 4)))

    def chain(names, x, th, tw, stride, post=None):
        """mres_can_chain: the residual blocks of one shape run as ONE launch where the frame fits the tile."""
        if H // stride <= th and W // stride <= tw:
            groups = [names]
        else:
            groups = [[n] for n in names]
        for g in groups:
            last = g is groups[-1]
            layers = tuple(l for n in g for l in _res(n)) + ((post,) if post and last else ())
            out = post if post and last else g[-1]
            internal = _internal(layers, g, (out,))
            kind = "mres" + (".chain" if len(g) > 1 else "") + (".post" if post and last else "")
            add(kind, layers, [x], [out], k_mres([_res(n) for n in g], True, post=post if last else None), internal=internal, tiles=((th, tw),))
            x = out
        return x

    x = chain(["res4_1", "res4_2", "res4_3", "res4_4"], x, 16, 20, 16)
    add("mres.wexp", ("conv4_2", "conv4_3", "conv5_1"), [x], ["conv5_1", "conv4_2"], k_mres([("conv4_2", "conv4_3", "conv5_1")], False, wexp=True),
        internal=("conv4_3",), tiles=((8, 10), (8, 4)))
    x = chain(["res5_1", "res5_2", "res5_3", "res5_4", "res5_5"], "conv5_1", 8, 10, 32, post="conv5_2" if deep else None)
    if not deep:
        add("pw", ("conv5_2",), [x], ["conv5_2"], k_pw("conv5_2"))
    if deep and H // 32 <= 8 and W // 32 <= 10:      # mdw2_can_chain
        add("mdw2", ("conv5_3", "conv5_4", "conv5_5", "conv5_6", "head_5"), ["conv5_2"], ["head_small"],
            k_mdw([("conv5_3", "conv5_4"), ("conv5_5", "conv5_6")], "head_5"), internal=("conv5_3", "conv5_4", "conv5_5", "conv5_6"), tiles=((8, 10),))
    else:
        add("mdw", ("conv5_3", "conv5_4"), ["conv5_2"], ["conv5_4"], k_mdw([("conv5_3", "conv5_4")], None), internal=("conv5_3",), tiles=((16, 20), (8, 10)))
        add("mdw.head", ("conv5_5", "conv5_6", "head_5"), ["conv5_4"], ["head_small"], k_mdw([("conv5_5", "conv5_6")], "head_5"),
            internal=("conv5_5", "conv5_6"), tiles=((16, 20), (8, 10)))
    if deep:
        add("dcat", ("deconv5_1", "conv4_1_1"), ["conv5_2", "conv4_2"], ["conv4_1_1"], k_dcat(), internal=("deconv5_1",))
    else:
        add("pw", ("deconv5_1",), ["conv5_2"], ["deconv5_1"], k_pw("deconv5_1"))
        add("pw", ("conv4_1_1",), ["conv4_2", "deconv5_1"], ["conv4_1_1"], k_pw("conv4_1_1"))
    add("mdw", ("conv4_1_2", "conv4_1_3"), ["conv4_1_1"], ["conv4_1_3"], k_mdw([("conv4_1_2", "conv4_1_3")], None), internal=("conv4_1_2",),
        tiles=((16, 20), (8, 10)))
    add("mdw.head", ("conv4_1_4", "conv4_1_5", "head_4"), ["conv4_1_3"], ["head_large"], k_mdw([("conv4_1_4", "conv4_1_5")], "head_4"),
        internal=("conv4_1_4", "conv4_1_5"), tiles=((16, 20), (8, 10)))
    return T


KINDS = ("valu", "k19h", "mres", "mres.wexp", "mres.chain", "mres.post", "mres.chain.post", "pw", "dcat", "mdw", "mdw.head", "mdw2")


def run(launch, net, inputs, dtype):
    """One launch from the given input tensors (dict name -> tensor, any float dtype) in `dtype` -> dict name -> output."""
    with torch.no_grad():
        outs = launch.fn(net, tuple(inputs[n].to(dtype) for n in launch.inputs))
    return dict(zip(launch.outputs, outs))


def chained(table, net, x, dtype=torch.float32):
    """All launches in order, each from its predecessors' outputs -> every tensor of the plan."""
    t = {"input": x.to(dtype)}
    for L in table:
        t.update(run(L, net, t, dtype))
    return t


# ---- the comparator --------------------------------------------------------------------------------------------------------------------
#
# Two correct evaluations of a launch (another summation order in fp32) differ in three ways:
#   1. the output's own rounding: an fp32 sum within its accumulation error of a rounding boundary goes the other way -- ONE fp16 ulp;
#   2. cancellation: an output that is a thousandth of the terms it is the sum of carries their fp32 error, which is many ulps OF THE RESULT
#      (measured on the CPU: up to 89 ulps in the stem, where no launch-internal rounding exists at all) but a fraction of an fp16 ulp at the
#      terms' size;
#   3. a flipped rounding INSIDE the launch (E, A): the operand moves by one of ITS fp16 ulps, every output it feeds by |w| times that.
# So the distance is counted in fp16 ulps at max(|exact|, M), M = sum |w| |x| + |b| (+ |residual|) of the launch's last conv: the size of the
# terms the element is the sum of.  In that unit the float32 twin stays within 1.0 of the float64 replay in every launch kind but the
# chains (1.8).  The figure in the result's own ulps (floor 2^-14) is reported beside it; it is not a criterion (2200 for k19h_kernel's model
# against itself).
# Chained launches: a block's result stays in LDS as fp32 and the NEXT expansion rounds it as its operand.  Of those roundings one in ~10^4
# falls the other way in another evaluation, moves 136 / 224 expanded channels of its pixel and with them all channels of the 3x3 pixels
# around it by about one ulp: 8 .. 32 % of a chain's output elements differ between twin and float64 (single blocks: <= 0.6 %).  Bit equality is
# therefore no criterion for a chain; its "differs" is "further than half an fp16 ulp at the terms' size" (twin: <= 0.35 % of the elements).

def ulp16(a):
    """One fp16 ulp at |a| (float64 array), subnormals counted as the smallest normal's: 2^(floor(log2 max(|a|, 2^-14)) - 10)."""
    m = np.maximum(np.abs(a), 2.0 ** -14)
    return np.exp2(np.floor(np.log2(m)) - 10)


@dataclasses.dataclass
class Cmp:
    share: float            # share of elements with got != rne16(exact64) (fp32 outputs: with |got - exact64| > 2e-5 max(1, max |exact64|))
    far: float              # share of elements further than half an fp16 ulp at the terms' size
    dist: float             # largest |got - exact64| in fp16 ulps at max(|exact64|, terms' size)
    ulps: float             # largest |got - exact64| in fp16 ulps of max(|exact64|, 2^-14): reported only
    n_diff: int
    where: str              # the worst offenders and what they have in common


def compare(got, exact64, scale64=None, tiles=(), fp32=False, far_only=False, top=5) -> Cmp:
    g = got.detach().cpu().double().numpy()
    e = exact64.detach().cpu().double().numpy()
    assert g.shape == e.shape and e.ndim == 4, (g.shape, e.shape)
    m = np.abs(e) if scale64 is None else np.maximum(np.abs(e), scale64.detach().cpu().double().numpy())
    err = np.abs(g - e)
    dist = err / ulp16(m)
    far = dist > 0.5
    if fp32:
        bad = err > F32_RTOL * max(1.0, float(np.abs(e).max()))
    else:
        bad = g != e.astype(np.float16).astype(np.float64)
    c = Cmp(float(bad.mean()), float(far.mean()), float(dist.max()), float((err / ulp16(e)).max()), int(bad.sum()), "")
    mark = far if far_only else bad
    if mark.any():
        N, C, Hh, Ww = e.shape
        idx = np.argwhere(mark)
        order = np.argsort(-dist[mark], kind="stable")[:top]
        n, ch, y, x = idx.T
        border = (y == 0) | (y == Hh - 1) | (x == 0) | (x == Ww - 1)
        seam = np.zeros(len(idx), bool)
        for th, tw in tiles:
            seam |= ((y % th == 0) | (y % th == th - 1)) & (Hh > th) | ((x % tw == 0) | (x % tw == tw - 1)) & (Ww > tw)
        worst = ["(n=%d, c=%d, y=%d, x=%d): got %.6g, exact %.6g%s%s" % (*idx[i], g[tuple(idx[i])], e[tuple(idx[i])],
                                                                         ", border" if border[i] else "", ", tile seam" if seam[i] else "")
                 for i in order]
        ring = 1.0 - max(Hh - 2, 0) * max(Ww - 2, 0) / float(Hh * Ww)
        c.where = ("%d of %d elements; %.0f %% of them on the border rows / columns (%.0f %% of the tensor lie there), %.0f %% on a tile seam of %s; "
                   "per frame %s; busiest channel %d with %d; last column %d, last row %d; worst: %s"
                   % (len(idx), e.size, 100 * border.mean(), 100 * ring, 100 * seam.mean(), list(tiles), np.bincount(n, minlength=N).tolist(),
                      int(np.bincount(ch).argmax()), int(np.bincount(ch).max()), int((x == Ww - 1).sum()), int((y == Hh - 1).sum()), "; ".join(worst)))
    return c


def is_chain(kind):
    return ".chain" in kind


def by_distance(launch):
    """Launches whose "differs" is "further than half an fp16 ulp at the terms' size": the chains (see above) and the two head launches.  The
    heads are fp32, but their operand is rounded to fp16 inside the launch (A); where that rounding falls the other way a logit moves by up
    to 2^-10 of one term, which is outside the fp32 criterion (2e-5 of the logits' range) whenever a term exceeds 2 % of the range: 2.4 %
    of the small head's logits with the seeded random weights, twin against float64.  The share outside the fp32 criterion is held to the
    margin times the twin's own as a third criterion (F32_REFERENCE), without the 2 % cap, which the twin itself exceeds there."""
    return is_chain(launch.kind) or launch.fp32_out


def check(launch, out_name, got, exact64, scale64):
    """Compare one output of one launch; -> (Cmp, the share its kind is held to)."""
    c = compare(got, exact64, scale64, launch.tiles, fp32=launch.fp32_out, far_only=by_distance(launch))
    return c, (c.far if by_distance(launch) else c.share)


def limits(kind, reference):
    """The criteria of one launch kind from the reference-against-itself figures (share, distance) of that kind: the margin times the share
    and never more than 2 %; the distance + 1 ulp and never more than 8."""
    share, dist = reference[kind]
    return min(MARGIN * share, SHARE_CAP), min(dist + 1.0, ULP_CAP)


def verdict(launch, out_name, c: Cmp, reference):
    """None if the tensor passes the criteria, else the assertion text: which launch, which tensor, where."""
    smax, dmax = limits(launch.kind, reference)
    share = c.far if by_distance(launch) else c.share
    f32max = MARGIN * F32_REFERENCE[launch.kind] if launch.fp32_out else 1.0
    if share <= smax and c.dist <= dmax and (not launch.fp32_out or c.share <= f32max):
        return None
    what = "are further than half an fp16 ulp (at the size of the summed terms) from the exact value" if by_distance(launch) else "differ from rne16(exact)"
    if launch.fp32_out:
        what += " and %.3f %% are further than 2e-5 of the range (limit %.3f %%)" % (100 * c.share, 100 * f32max)
    return ("launch %s [%s] -> %s: %.3f %% of the elements %s (limit %.3f %%), largest distance %.2f fp16 ulps at the terms' size (limit %.2f; "
            "%.0f in the result's own ulps); %s" % (launch.name, launch.kind, out_name, 100 * share, what, 100 * smax, c.dist, dmax, c.ulps, c.where))


def replay_and_check(launch, net, tensors, got, reference=None):
    """The float64 replay of one launch from `tensors` (its inputs) against `got` (its outputs) -> [(out_name, Cmp, share, verdict)]."""
    net.scale = None
    exact = run(launch, net, tensors, torch.float64)
    res = []
    for (name, e), m in zip(exact.items(), net.scale):
        c, share = check(launch, name, got[name], e, m)
        res.append((name, c, share, verdict(launch, name, c, reference) if reference is not None else None))
    return res


# What the float32 twin differs from the float64 replay by, per launch kind: the worst share of differing elements (chains: of elements
# further than half an ulp at the terms' size; fp32 outputs: outside the fp32 criterion) and the largest distance, over the whole
# parametrisation of the GPU test.  tests/test_cpu_f16_replay.py::test_reference_against_itself measures them again, asserts that none is
# exceeded and that each is within the caps; the header table of that file has the figures as measured, beside the GPU's.
REFERENCE: Dict[str, Tuple[float, float]] = {
    "valu": (0.0056, 1.0), "k19h": (0.00215, 1.0), "mres": (0.00274, 1.0), "mres.wexp": (0.00106, 1.0), "mres.chain": (0.00348, 1.82),
    "mres.post": (0.00119, 0.5), "mres.chain.post": (0.00035, 1.0), "pw": (0.00061, 1.0), "dcat": (0.00157, 0.5), "mdw": (0.0033, 1.0),
    "mdw.head": (0.0, 0.33), "mdw2": (0.0, 0.42),
}
F32_REFERENCE: Dict[str, float] = {"mdw.head": 0.0132, "mdw2": 0.0238}   # the head launches: worst share of logits outside the fp32 criterion, twin against float64


# ---- inputs shared by the CPU and the GPU test -------------------------------------------------------------------------------------------

SIZES = ((96, 160), (160, 224), (256, 352))


def frames_u8(golden, H, W, N, seed=0):
    """Uniform-noise frames; frame 1 is a bundled test frame cropped to the size (realistic activation statistics)."""
    u8 = np.random.default_rng(1000 * H + W + seed).integers(0, 256, size=(N, H, W), dtype=np.uint8)
    big = golden("golden_512")["input_u8"][3]
    u8[1] = big[64:64 + H, 96:96 + W]
    return u8


# (H, W, N): partial tiles everywhere; the stride-16 / 32 frames fit one tile; one column of tiles more than the chains allow.  Batches: 2
# takes every launcher's few-frames tiling; the large one takes the many-frames tiling -- the launchers switch at 2 N tiles <= #CU (256 CUs;
# mres_small_batch and its likes), i.e. above 128 frames where a frame is one tile and above 32 where it is four.  (The split-sum launches
# and launch_mres's block-by-block form, which switch at 9 frames, do not exist for fp16 storage.)
CASES = ((96, 160, 2), (96, 160, 132), (160, 224, 2), (160, 224, 36), (256, 352, 2))


def state_dicts():
    import os
    from tests.random_weights import random_state_dict
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    shipped = os.path.join(root, "yolo-fastest-and-embedded-deployment_amd", "assets", "weights", "yolo_fastest_256x320_epoch28.pth")
    return {"shipped": lambda: bo.load_state_dict(shipped), "random": lambda: random_state_dict(0)}
