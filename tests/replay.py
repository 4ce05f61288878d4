"""TEST INFRASTRUCTURE (CPU only but for `collect`, never imported by the product): the forward plan replayed ONE LAUNCH AT A TIME, in all three
precisions of the engine: the fp16-storage plan (`precision` "f16") against a model that rounds where the kernel rounds, the fp32-storage
plans ("f32" and "f16x3") against the plain float64 evaluation of the launch.

The head-level bounds of tests/test_gpu_parity.py are 2 .. 4 fp16 ulps at the heads and hundreds of ulps at an interior tensor (fp16), or
3 x torch's own fp32 error (fp32), because 86 layers of legitimate rounding have accumulated there.  Here the accumulation is removed: every
launch of the plan is evaluated in float64 from the input tensor(s) the GPU itself produced, and the GPU's output is compared with it
element by element.
  f16          The inputs are fp16 values, exactly representable; the float64 replay rounds to nearest even to fp16 at exactly the places
               where that launch rounds.  The unit is an fp16 ulp: anything below 2.4e-4 relative is invisible to it.
  f32, f16x3   A launch has NO rounding point: fp32 storage keeps every tensor as the kernel computed it, so the exact value of a launch is
               its float64 evaluation, and the distance of the GPU's output from it is counted in fp32 ulps at the size of the terms the
               element is the sum of (M = sum |w| |x| + |b| (+ |residual|) of the launch's last conv, `magnitude`).
The same launch functions run on float32 tensors (the "twin", torch CPU): twin against float64 is the reference's own noise and sets the
scale of the GPU criteria.  tests/test_cpu_f16_replay.py and tests/test_cpu_plan_replay.py measure it; tests/test_gpu_f16_replay.py and
tests/test_gpu_plan_replay.py hold the device to 3 x the twin's figure (fp32: and never to more than the a-priori bound, `cap`).  The fp16
twin chained over the whole net is bitwise `oracle.fp16_rounding_sim.Sim(W, T, A, E, size, fusion)`.

WEIGHTS.  `packer.pack_state_dict` folds BatchNorm in float64 (`fold_bn`) and rounds ONCE to fp32; the engine packs fp16 fragments from those
fp32 values with `f32_to_f16_bits` (RNE; yf_mfma_kernels.hip).  `Net` unpacks the blob the engine is given, so the fp32 values are the GPU's.
Biases and depthwise weights stay fp32 in every kernel ("b1 / wd / bd / b2 stay fp32", yf_mres_kernels.hip mres_pack_weights).

THE LAUNCH TABLE (`launch_table`), from yf_engine.hip build_plan and the launchers.  build_plan does not depend on the dtype
(mres_has_kernel ignores its dtype argument), so the launches, their layers, inputs, outputs and on-chip tensors are stated once; the
kernels, the forms and what each is handed depend on the precision:

  fusion 0    f32 / f16x3 only: run_forward refuses fp16 storage ("fp16 storage needs a fused plan", yf_engine.hip).  One launch per layer
              (Builder::unit): conv0 and conv1_9 on dense3x3s2 (`l.dense`), depthwise on launch_dw (`l.dw`), every 1x1 conv, the deconv and
              the two head convs on launch_pw (`l.pw`, `l.dc`, `l.head`): the fp32 VALU kernels of yf_conv_kernels.hip.  yf_create_ex packs
              MFMA fragments for plans 1 and 2 only (`for (int lvl = 1; lvl <= 2; ++lvl)`), so plan 0 never reaches launch_pw_mfma, and it
              hands every op the STORAGE dtype (`o.kdt = e->sdt()`): DT_F32 in an f16x3 engine.
  fusion 1/2  in the fp32-storage engines on other kernels and in other forms than with fp16 storage:
    valu[.stem] fused_block_kernel<float>: the stem (conv0 in front), res1_1, res2_1, res2_2.  DT_F32 in every fp32-storage engine
                (launch_fused_block has no x3 form).  fp16: fused_block_kernel<.., half_t>, kind `valu` for all four.
    k19h        f16 engine: k19h_kernel.
    k19r        f32 engine: k19r_kernel<8, false> (items <= 64 #CU) or <16, true>.
    k19m        f16x3 engine: k19m_kernel, NOT k19r_kernel (launch_k19m: "DT_F16X3: the region-buffer kernel").  conv1_8 is an exact fp32
                MFMA; its result is split once; conv1_9 and conv2_1 issue three products each.
    mres        mres_kernel / mres_pc_kernel<half_t | float | x3_t>, one block.  Few frames (`mres_small_batch`: 2 N tiles <= #CU):
                res3_3..6 on 8x10 tiles, the conv3_5 and conv4_2 triples on 8x4 output tiles.
    mres.wexp   conv4_2+conv4_3+conv5_1, conv4_2 written as well.
    mres.chain  res4_1..4 / res5_1..5 as one launch, one dispatch (mres_can_chain: frames that fit one tile).
    mres.unchained   the res4 chain at few frames: launch_chain_unchained, nblk dispatches on 8x10 tiles through the unnamed scratch tensor
                (not probe-able: the op is replayed as one unit).  f32 and f16x3.
    mres.esplit[.post]   the res5 chain at 8x10 with N <= ESPLIT_MAX_FRAMES, f32 engine only (mres_esplit_ok: `dtype == DT_F32`): nblk + 1
                dispatches of mres_esplit_kernel; at fusion 2 conv5_2 rides in the last one.
    mres[.chain].post    fusion 2: conv5_2 on the last res5 block's result in LDS, fp32 MFMAs in every engine (mres_post_conv).
    pw          fusion 1: conv5_2, deconv5_1, conv4_1_1.  fp16: pw_mfma_kernel<.., half_t>.  fp32 storage: all three shapes are in
                YF_WS_SHAPES, so launch_pw_mfma sends them to pw_ws_kernel / pw_ws_x3_kernel (`dtype != DT_F16`); pw_mfma_kernel<float> is
                not reached by any plan of the shipped shapes.
    dcat        fusion 2: dcat_h_kernel / dcat_kernel / dcat_x3_kernel; the latter two <1> at few frames (2 N ceil(hw / 80) <= #CU), else
                <DC_MT>.
    mdw, mdw.head   mdw_kernel<half_t | float | x3_t>; fp32 storage: the stride-16 pair on 8x10 tiles at few frames.
    mdw2        fusion 2, frames that fit one 8x10 tile.
    mdw2.esplit f32 engine, 8x10 exactly, N <= MDW2_ESPLIT_MAX_FRAMES: three dispatches of mdw2_esplit_kernel.
  Other io_params than the shipped ones (`launch_table(..., num_out, input_channel)`; the section at the end of this file): more than four
  input planes put conv0 in front of the fused plans as a launch of its own (`l.dense`: conv0_any_kernel<float | half_t>) with the pre = false
  block conv1_2+conv1_3+conv1_4 behind it (`valu`); heads wider than 32 channels take mdw_kernel's head mode 2 and never the one-launch small head.
  The few-frames split-sum launches and launch_mres's block-by-block form are fp32-storage only (`dtype != DT_F16`, `dtype == DT_F32`): with
  fp16 storage a batch size only selects tile shapes (`mres_small_batch`: 2 N tiles <= #CU).

THE CONTEXT (`Ctx`) owns where a (precision, mode) pair rounds; the launch functions (`k_*`) are the kernels' dataflow.  mode `exact` is
float64, mode `twin` float32.

ROUNDING POINTS PER LAUNCH KIND, fp16 storage (W = weights of an MFMA layer rounded, A = activation operand of a pointwise MFMA rounded:
both are `Ctx.gemm`; T = tensor written to HBM rounded: `Ctx.stored`; E: `Ctx.on_chip`; everything else is fp32 arithmetic on fp32 values,
`Ctx.fp32`, modelled in float64):

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

THE fp32-STORAGE TWINS.  `f32`: the launch in torch float32 on the CPU; nothing is rounded anywhere.  `f16x3`: what the x3 kernels were found
to issue, which is the same in all of them (mres_kernel, mres_pc_kernel, mdw_kernel, mdw2_kernel, pw_ws_x3_kernel, dcat_x3_kernel,
k19m_kernel):
  * the activation operand of a pointwise / dense GEMM is split where it is produced: hi = rne16(a), lo = rne16(a - hi), a - hi exact in
    fp32 (yf_kernels.h split_f16x4); the weights on the host: hi = f32_to_f16_bits(w), lo = f16_lo_bits(w) -- the same two roundings;
  * THREE products per k-block, w_lo a_hi + w_hi a_lo + w_hi a_hi, accumulated in fp32 in that order; lo lo is never issued;
  * bias (and residual) are added in fp32 after the GEMM; depthwise convs, the stem / res1 / res2 blocks and conv5_2 inside the res5 launch
    are fp32 arithmetic on fp32 values (the f32 twin);
  * fp16 subnormal operands are KEPT by the MFMA (tools/mfma16_probe.hip; DESIGN_HISTORY.md): lo is subnormal for every operand below 1/8,
    so the twin rounds with gradual underflow (torch's float -> half) and flushes nothing.
"""
import ctypes
import dataclasses
from typing import Callable, Dict, List, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle import backbone_oracle as bo

LAYER = dict(bo._BY_NAME)
for _h, _cin in (("head_5", 128), ("head_4", 96)):
    LAYER[_h] = (_h, "head", _cin, 24, 1, 1, False)


def layers_for(num_out=24, input_channel=1):
    """The layer records of a configuration: io_params change conv0's `cin` and the two head convs' `cout` and nothing else.  `lin` and the
    launch functions read kind, kernel size and stride only, which no configuration changes; `n_terms` needs conv0's fan-in."""
    if (num_out, input_channel) == (24, 1):
        return LAYER
    ly = dict(LAYER)
    ly["conv0"] = ly["conv0"][:2] + (input_channel,) + ly["conv0"][3:]
    for h in ("head_5", "head_4"):
        ly[h] = ly[h][:3] + (num_out,) + ly[h][4:]
    return ly


PRECISIONS = ("f16", "f32", "f16x3")
FP32_STORAGE = ("f32", "f16x3")
DT = {"f32": 0, "f16": 1, "f16x3": 2}
MARGIN = 3.0                       # the GPU's summation tree is a third association of the same sums
ESPLIT_MAX_FRAMES = 9              # yf_mres_kernels.hip, yf_mdw_kernels.hip (MDW2_ESPLIT_MAX_FRAMES)
REPLAY_THREADS = 16                # the CPUs a test run may use, not os.cpu_count()
# fp16: what the GPU criteria are multiples of: test_cpu_f16_replay.py measures the float32 twin against the float64 replay per launch kind
# over the whole parametrisation and asserts that nothing exceeds these (share of elements that differ, largest distance in fp16 ulps)
SHARE_CAP, ULP_CAP = 0.02, 8.0
F32_RTOL = 2e-5                    # fp32 outputs of the fp16 plan (the heads): test_layer_probes_match_reference's criterion for one launch


def cap_threads():
    """What the four replay test files do on import: a float64 replay on every CPU of a large host only slows itself down."""
    torch.set_num_threads(min(torch.get_num_threads(), REPLAY_THREADS))


def rne16(t):
    """Round to nearest even to fp16, dtype kept.  float64 goes through numpy: torch's double -> half converts through float (double rounding)."""
    if t.dtype == torch.float64:
        return torch.from_numpy(t.numpy().astype(np.float16).astype(np.float64))
    return t.half().to(t.dtype)


def split16(t):
    """hi = rne16(t), lo = rne16(t - hi), as float32 (split_f16x4; gradual underflow, nothing flushed)."""
    hi = t.half().float()
    return hi, (t - hi).half().float()


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
        self.perturb = {}    # the CPU tests: planted defects of the twin, keyed as `Ctx` lists them
        self.records = layers_for(num_out, input_channel)

    def w(self, dtype, name, rounded):
        key = (dtype, name, rounded)
        if key not in self._cache:
            w, b = self.f32[name]
            self._cache[key] = ((rne16(w) if rounded else w).to(dtype), b.to(dtype))
        return self._cache[key]


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
        self._cache, self.perturb, self.records = {}, {}, LAYER


def dw64(x, w, b, k, s):
    """Depthwise conv as shifted multiply-adds (torch's float64 grouped conv is a slow generic path)."""
    p = (k - 1) // 2
    xp = F.pad(x, (p, p, p, p))
    Ho, Wo = (x.shape[2] + 2 * p - k) // s + 1, (x.shape[3] + 2 * p - k) // s + 1
    y = b.view(1, -1, 1, 1).expand(x.shape[0], -1, Ho, Wo).clone()
    for ky in range(k):
        for kx in range(k):
            y += xp[:, :, ky:ky + (Ho - 1) * s + 1:s, kx:kx + (Wo - 1) * s + 1:s] * w[:, 0, ky, kx].view(1, -1, 1, 1)
    return y


def lin(name, x, w, b=None):
    """The linear part of layer `name` (no ReLU) in x's dtype: oracle/fp16_rounding_sim.py Sim.unit's calls, so that the fp16 twin is bitwise Sim."""
    _, kind, cin, cout, k, s, relu = LAYER[name]
    if kind == "dc":
        return F.conv_transpose2d(x, w, b, stride=2)
    if kind == "dw" and x.dtype == torch.float64:
        return dw64(x, w, b if b is not None else torch.zeros(cout, dtype=x.dtype), k, s)
    return F.conv2d(x, w, b, stride=s if kind != "head" else 1, padding=(k - 1) // 2, groups=(x.shape[1] if kind == "dw" else 1))


def magnitude(net, name, x, W=False, res=None):
    """sum |w| |x| + |b| (+ |residual|) of the conv `name`: the size of the terms whose sum an output element is, i.e. what an fp32
    evaluation of it rounds at (float64)."""
    w, b = net.w(torch.float64, name, W)
    y = lin(name, x.double().abs(), w.abs(), b.abs())
    return y if res is None else y + res.double().abs()


def n_terms(layers, x3_layers=(), records=None):
    """Sum over the layers of the number of terms an output sums (taps x input channels + bias (+ residual, the blocks' conv3)); four times
    that for a split-operand GEMM: 22 kept operand bits against 24.  records: `layers_for` of another configuration than the shipped one."""
    t = 0.0
    for n in layers:
        _, kind, cin, cout, k, s, relu = (records or LAYER)[n]
        terms = (k * k if kind == "dw" else cin if kind in ("dc", "head") else cin * k * k) + 1 + (1 if n.endswith(".conv3") else 0)
        t += terms * (4.0 if n in x3_layers else 1.0)
    return t


class Ctx:
    """Where one (precision, mode) pair rounds, the size of the terms of the launch's outputs, and every planted defect.

    mode 'exact' (float64) never makes a mistake; mode 'twin' (float32) makes those of `net.perturb`:
      drop_tap {layer, ky, kx}         a depthwise layer omits one tap on the last output column
      halo_frame {layer, tile_h}       ... reads the halo row below the first row of tiles of frame 1 from frame 0
      tap_scale {layer, ky, kx, rel}   ... has one tap's weight off by `rel` on the last output column
      bias16 = layer                   the bias rounded to fp16 before it is added
      skip_a = layer                   f16: the A rounding of this GEMM's operand skipped
      late_bias = layer                f16: an output GEMM's bias added after the T rounding of its result
      swap_channels {pair}             two channels of the tensor rounded on chip (conv1_8 in k19h) swapped
      no_lo_hi = layer                 f16x3: w_lo a_hi left out
      flush_lo = layer                 f16x3: lo = 0 for operands below the smallest normal fp16 (changes no bit: test_cpu_plan_replay.py)
      flush_subnormal_lo = layer       f16x3: a lo half that is an fp16 subnormal taken as 0 (an MFMA that flushed)
    the io-dependent launches (tests/test_cpu_io_replay.py):
      head_last_is_padding = head      the last real head column takes the first padding column's value (zero weights, zero bias)
      head_pair_skipped = head         HM2: the second pair of column tiles never runs its k-loop: channels 32..63 keep the bias only
      head_bias_tile_local = head      HM2: the bias of a column past the first pair of tiles is read at its tile-pair-local index
      head_kblock_missing {head, tile, kblock}   one 16-column head tile sums its k-blocks with one 16-channel block left out
      swap_planes {pair}               conv0 reads two input planes swapped
    """

    def __init__(self, net, precision, mode, bound=False):
        assert precision in PRECISIONS and mode in ("exact", "twin")
        self.net, self.precision, self.exact = net, precision, mode == "exact"
        self.dtype = torch.float64 if self.exact else torch.float32
        self.perturb = {} if self.exact else net.perturb
        self.scale = {}      # exact: output index -> the size of the terms of the launch's output (`out=` of the conv that makes it)
        # exact fp32: id(tensor) -> (tensor, its propagated a-priori error bound), see `cap`; `bound` = that of the launch's result
        self.B = {} if (bound and self.exact and precision != "f16") else None
        self.bound = None
        self._late = None

    def _epilogue(self, name, y, res):
        if res is not None:
            y = y + res
        return F.relu(y) if LAYER[name][6] else y

    def _bias(self, name, b):
        return b.half().to(b.dtype) if self.perturb.get("bias16") == name else b

    def gemm(self, name, x, res=None, out=None, f16_only=False):
        """A GEMM on the matrix cores (+ bias (+ residual) (+ ReLU) in fp32): W and A rounded for f16, the three split products for the f16x3
        twin, plain otherwise.  out: the result is output `out` of the launch -- its terms' size is taken, on the operand the GEMM receives.
        f16_only: only k19h_kernel runs this one on fp16 operands (conv1_8, K = 4: fp32 VALU in k19r, one exact fp32 MFMA k-step in k19m)."""
        f16, p = self.precision == "f16", self.perturb
        if f16_only and not f16:
            return self.fp32(name, x, res, out)
        w, b = self.net.w(self.dtype, name, f16)
        b = self._bias(name, b)
        if f16 and p.get("skip_a") != name:
            x = rne16(x)
        if self.exact and out is not None:
            self.scale[out] = magnitude(self.net, name, x, W=f16, res=res)
        if self.precision == "f16x3" and not self.exact:
            (wh, wl), (xh, xl) = split16(w), split16(x)
            if p.get("flush_lo") == name:
                wl = torch.where(w.abs() < 2.0 ** -14, torch.zeros_like(wl), wl)
                xl = torch.where(x.abs() < 2.0 ** -14, torch.zeros_like(xl), xl)
            if p.get("flush_subnormal_lo") == name:
                wl = torch.where(wl.abs() < 2.0 ** -14, torch.zeros_like(wl), wl)
                xl = torch.where(xl.abs() < 2.0 ** -14, torch.zeros_like(xl), xl)
            y = lin(name, xl, wh) + lin(name, xh, wh)
            if p.get("no_lo_hi") != name:
                y = lin(name, xh, wl) + y
            y = y + b.view(1, -1, 1, 1)
        elif f16 and out is not None and p.get("late_bias") == name:
            y = self._epilogue(name, lin(name, x, w), res)
            self._late = (y, b)                                        # `stored` rounds, THEN adds the bias
            return y
        else:
            y = lin(name, x, w, b)
        if LAYER[name][1] == "head" and p:
            y = self._head_defects(name, x, w, b, y)
        return self._epilogue(name, y, res)

    def _head_defects(self, name, x, w, b, y):
        """The planted errors of the head conv chained into mdw_kernel / mdw2_kernel (see the class comment); w [num_out, cin, 1, 1]."""
        p, n = self.perturb, w.shape[0]
        if p.get("head_last_is_padding") == name:
            y = y.clone()
            y[:, n - 1] = 0.0
        if p.get("head_pair_skipped") == name:
            assert n > 32
            y = y.clone()
            y[:, 32:min(n, 64)] = b[32:min(n, 64)].view(1, -1, 1, 1)
        if p.get("head_bias_tile_local") == name:
            assert n > 32
            idx = torch.arange(n)
            y = y + (b[idx % 32] - b).view(1, -1, 1, 1)
        q = p.get("head_kblock_missing")
        if q and q["head"] == name:
            cols = slice(16 * q["tile"], min(16 * q["tile"] + 16, n))
            ks = slice(16 * q["kblock"], 16 * q["kblock"] + 16)
            y = y.clone()
            y[:, cols] -= F.conv2d(x[:, ks], w[cols, ks])
        return y

    def fp32(self, name, x, res=None, out=None):
        """fp32 arithmetic on fp32 values in every precision: depthwise layers, the VALU blocks, the per-layer plan, conv5_2 inside the res5
        launch, conv1_8 outside fp16."""
        w, b = self.net.w(self.dtype, name, False)
        b = self._bias(name, b)
        if name == "conv0" and self.perturb.get("swap_planes"):
            i, j = self.perturb["swap_planes"]["pair"]
            x = x.clone()
            x[:, [i, j]] = x[:, [j, i]]
        if self.exact and out is not None:
            self.scale[out] = magnitude(self.net, name, x, res=res)
        y = lin(name, x, w, b)
        if LAYER[name][1] == "dw":
            y = self._dw_defects(name, x, w, b, y)
        y = self._epilogue(name, y, res)
        if self.B is not None:                                         # |dy| <= |w| |dx| (+ |dres|) + terms x ulp32(M); ReLU is 1-Lipschitz
            by = torch.from_numpy(ulp32(magnitude(self.net, name, x, res=res).numpy())) * n_terms([name], records=self.net.records)
            if id(x) in self.B:
                by = by + lin(name, self.B[id(x)][1], w.abs())
            if res is not None and id(res) in self.B:
                by = by + self.B[id(res)][1]
            self.B[id(y)] = (y, by)
            self.bound = by
        return y

    def _dw_defects(self, name, x, w, b, y):
        def mine(key):
            p = self.perturb.get(key)
            return p if p and p["layer"] == name else None
        p = mine("drop_tap")
        if p:
            w2 = w.clone()
            w2[:, 0, p["ky"], p["kx"]] = 0
            y = y.clone()
            y[..., -1] = lin(name, x, w2, b)[..., -1]
        p = mine("halo_frame")
        if p:
            th = p["tile_h"]
            assert x.shape[0] >= 2 and x.shape[2] > th and LAYER[name][5] == 1
            x2 = x.clone()
            x2[1, :, th] = x[0, :, th]
            y = y.clone()
            y[1, :, th - 1] = lin(name, x2, w, b)[1, :, th - 1]
        p = mine("tap_scale")
        if p:
            w2 = w.clone()
            w2[:, 0, p["ky"], p["kx"]] *= 1.0 + p["rel"]
            y = y.clone()
            y[..., -1] = lin(name, x, w2, b)[..., -1]
        return y

    def on_chip(self, t):
        """A tensor rounded on chip: E of k19h_kernel, the one expanded tensor of the fp16 plan that is rounded."""
        t = rne16(t) if self.precision == "f16" else t
        p = self.perturb.get("swap_channels")
        if p:
            i, j = p["pair"]
            t = t.clone()
            t[:, [i, j]] = t[:, [j, i]]
        return t

    def stored(self, t):
        """A tensor as it is written to HBM: T for f16, as computed otherwise."""
        if self.precision != "f16":
            return t
        if self._late is not None and self._late[0] is t:
            return rne16(t) + self._late[1].view(1, -1, 1, 1)
        return rne16(t)


# ---- the launch kinds: fn(ctx, ins) -> outputs -------------------------------------------------------------------------------------------

def k_layer(name, res, gemm):
    """One layer as a launch: the per-layer plan (fp32 VALU kernels) and the `pw` launches of fusion 1 (MFMA)."""
    def fn(c, ins):
        if res:
            x, r = ins[0], ins[-1]
        else:
            x, r = (ins[0] if len(ins) == 1 else torch.cat(ins, 1)), None
        return (c.stored((c.gemm if gemm else c.fp32)(name, x, res=r, out=0)),)
    return fn


def k_valu(layers, res):
    def fn(c, ins):
        (x,) = ins
        y = x
        for n in layers[:-1]:
            y = c.fp32(n, y)
        return (c.stored(c.fp32(layers[-1], y, res=x if res else None, out=0)),)
    return fn


def k_k19():
    def fn(c, ins):
        (x,) = ins
        y = c.on_chip(c.gemm("conv1_8", x, f16_only=True))
        y = c.gemm("conv1_9", y)
        return (c.stored(c.gemm("conv2_1", y, out=0)),)
    return fn


def k_mres(blocks, res, post=None, wexp=False):
    """blocks: [(expand, depthwise, project), ...] -- more than one = a chained launch: a block's result stays on chip, un-rounded."""
    def fn(c, ins):
        (x,) = ins
        for bi, (a, b, p) in enumerate(blocks):
            last = bi == len(blocks) - 1
            e = c.gemm(a, x, out=1 if wexp and last else None)
            d = c.fp32(b, e)
            x = c.gemm(p, d, res=x if res else None, out=0 if last and not post else None)
        if post:
            x = c.fp32(post, x, out=0)                 # conv5_2 on the un-rounded tile: fp32 MFMAs on fp32 weights in every engine
        return (c.stored(x), c.stored(e)) if wexp else (c.stored(x),)
    return fn


def k_dcat():
    def fn(c, ins):
        c52, c42 = ins
        d = c.stored(c.gemm("deconv5_1", c52))         # in registers, rounded as the deconv launch it replaces would store it
        return (c.stored(c.gemm("conv4_1_1", torch.cat((c42, d), 1), out=0)),)
    return fn


def k_mdw(pairs, head):
    """pairs: [(depthwise, pointwise), ...] -- two = mdw2_kernel, the first pair's result stays in LDS un-rounded."""
    def fn(c, ins):
        (x,) = ins
        for i, (d, p) in enumerate(pairs):
            y = c.fp32(d, x)
            x = c.gemm(p, y, out=0 if i == len(pairs) - 1 and not head else None)
        if head:
            return (c.gemm(head, x, out=0),)           # stored as fp32 NCHW in every precision
        return (c.stored(x),)
    return fn


# ---- the table ---------------------------------------------------------------------------------------------------------------------------

@dataclasses.dataclass
class Launch:
    name: str                     # the engine's name of the op: its layers joined by '+' (yf_op_info_ex)
    kind: str
    inputs: Tuple[str, ...]       # tensors that exist in device memory (yf_forward_probe)
    outputs: Tuple[str, ...]      # ... 'head_large' / 'head_small' are the forward's results, fp32
    internal: Tuple[str, ...]     # tensors of the reference module that this launch keeps on chip: YF_E_NOPROBE, replayed as part of it
    tiles: Tuple[Tuple[int, int], ...]   # output tile shapes the launch may use: where a seam would show
    fn: Callable
    dtype: int = 0                # what yf_op_dtype reports: the dtype the op's kernel is handed
    dispatches: int = 1           # what yf_op_dispatches reports at this batch
    form: str = ""                # the launcher's choice at this batch and CU count, restated (fp32 storage)
    terms: float = 0.0            # fp32 storage: the a-priori forward-error bound of the launch in fp32 ulps at the terms' size (see `cap`)

    @property
    def fp32_out(self):
        return self.outputs[0].startswith("head_")


def small_batch(N, H, W, th, tw, n_cu):
    """mres_small_batch and its likes: the larger tiling would leave more than half of the CUs idle."""
    return 2 * N * (-(-H // th)) * (-(-W // tw)) <= n_cu


def res_block(n):
    return (n + ".conv1", n + ".conv2", n + ".conv3")


def launch_table(H, W, fusion, precision, N=2, n_cu=256, split_sums=True, num_out=24, input_channel=1, head_forms=False) -> List[Launch]:
    """The launches of the plan of a `precision` engine for N frames of H x W on a device with n_cu compute units, in issue order (yf_engine.hip
    build_plan).  num_out = num_anchors * (5 + num_cls) and input_channel are the io_params the plan depends on (defaults: the shipped one
    input channel, 24 head channels):
      stem        2 .. 4 input planes: the same launch (fused_block_kernel<.., C0>); more: launch_fused_block returns -1 for pre_c0 > 4, so
                  build_plan issues conv0 as a launch of its own (conv0_any_kernel, handed the STORAGE dtype) and the pre = false block
                  conv1_2+conv1_3+conv1_4 behind it;
      small head  mdw2_can_chain / mdw2_esplit_ok: one launch only for 1 <= num_out <= 32; wider heads run mdw + mdw.head on 8x10 tiles;
      head mode   mdw_head_mode: HM1 = up to 32 head channels, one pair of column tiles; HM2 = any width, the run-time loop over pairs.
    head_forms: the form of the mdw / mdw.head entries is "<tile> HM<mode>" in every precision -- launch_mdw's tile rule does not look at the
    dtype, so it is restated for fp16 storage too (tests/test_{cpu,gpu}_io_replay.py assert it); without it the table is the one the
    plan-replay and f16-replay tests have always had, entry for entry."""
    assert precision in PRECISIONS and H % 32 == 0 and W % 32 == 0 and num_out >= 1 and 1 <= input_channel <= 64
    LY = layers_for(num_out, input_channel)
    HM = 1 if num_out <= 32 else 2
    F16, F32, X3 = (precision == p for p in PRECISIONS)
    if F16 and fusion not in (1, 2):
        raise ValueError("fp16 storage needs a fused plan: fusion 1 or 2 (yf_engine.hip run_forward refuses level 0)")
    assert fusion in (0, 1, 2)
    T: List[Launch] = []

    def add(kind, layers, ins, outs, fn, blocks=(), tiles=(), valu=False, dispatches=1, form="", fp32_layers=(), keep_form=False):
        """valu: an fp32 VALU kernel, handed DT_F32 in an f16x3 engine too; fp32_layers: not split-operand GEMMs in an x3 kernel;
        keep_form: the form is stated for fp16 storage as well."""
        # a tensor of the reference module inside the launch that is not its output is kept on chip (a block's conv3 is not a tensor of its
        # own: the engine names the sum after it by the block; the head convs' results are the forward's outputs)
        internal = tuple(n for n in tuple(layers) + tuple(blocks) if n not in outs and not n.endswith(".conv3") and not n.startswith("head_"))
        x3 = [n for n in layers if LAYER[n][1] != "dw" and n not in fp32_layers] if X3 and not valu else []
        T.append(Launch("+".join(layers), kind, tuple(ins), tuple(outs), internal, tuple(tiles), fn,
                        DT["f16"] if F16 else DT["f32"] if valu else DT[precision], dispatches,
                        "" if F16 and not keep_form else form,   # the fp16 launchers' small-batch rules are not restated: both tile shapes are listed
                        0.0 if F16 else n_terms(layers, x3, LY)))

    if fusion == 0:
        prev = "input"
        for name, kind, cin, cout, k, s, relu in list(bo.LAYERS) + [LY["head_5"], LY["head_4"]]:
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
            add(lk, (name,), ins, [out], k_layer(name, res, gemm=False), valu=True)
            prev = out
        # build_plan issues each head conv directly behind its branch: head_5 after conv5_6, head_4 last
        h5 = T.pop([L.name for L in T].index("head_5"))
        T.insert([L.name for L in T].index("conv5_6") + 1, h5)
        return T

    deep = fusion == 2

    def tiling(big, small, few=None):
        """(tiles, form) of a launch with two tile shapes.  The fp16 table lists both; the fp32 one the launcher's choice at this N (`few`: its
        few-frames condition; None: this launcher has the one tiling)."""
        if F16:
            return (big, small), ""
        if few is None:
            return (big,), ""
        return ((small,), "%dx%d" % small) if few else ((big,), "%dx%d" % big)

    def triple(kind, layers, x, tf, out=None):
        """A block of three layers as one launch, a residual block where its layers are one's."""
        out, res = out or layers[-1], layers[-1].endswith(".conv3")
        valu = kind.startswith("valu")
        add(kind, layers, [x], [out], k_valu(layers, res) if valu else k_mres([tuple(layers)], res), tiles=tf[0], valu=valu, form=tf[1])
        return out

    if input_channel <= 4:
        x = triple("valu" if F16 else "valu.stem", ("conv0", "conv1_2", "conv1_3", "conv1_4"), "input", (((32, 32),), ""))
    else:
        add("l.dense", ("conv0",), ["input"], ["conv0"], k_layer("conv0", False, gemm=False), valu=True)
        x = triple("valu", ("conv1_2", "conv1_3", "conv1_4"), "conv0", (((32, 32),), ""))
    x = triple("valu", res_block("res1_1"), x, tiling((32, 16), (16, 16)), out="res1_1")
    k19 = ("conv1_8", "conv1_9", "conv2_1")
    if F16:
        add("k19h", k19, [x], ["conv2_1"], k_k19(), tiles=((1, 16),))
    elif X3:
        add("k19m", k19, [x], ["conv2_1"], k_k19(), tiles=((8, 16),), fp32_layers=("conv1_8",))
    else:
        items = N * (H // 4) * (-(-(W // 4) // 16))
        add("k19r", k19, [x], ["conv2_1"], k_k19(), tiles=((1, 16),), form="8 waves" if items <= 64 * n_cu else "16 waves, LDS weights")
    x = "conv2_1"
    for n in ("res2_1", "res2_2"):
        x = triple("valu", res_block(n), x, tiling((32, 16), (16, 16), small_batch(N, H // 4, W // 4, 32, 16, n_cu)), out=n)
    x = triple("mres", ("conv2_2", "conv2_3", "conv3_1"), x, tiling((8, 10), (8, 4)))
    for n in ("res3_1", "res3_2"):
        x = triple("mres", res_block(n), x, tiling((16, 20), (8, 10)), out=n)
    x = triple("mres", ("conv3_2", "conv3_3", "conv3_4"), x, tiling((16, 20), (8, 10)))
    for n in ("res3_3", "res3_4", "res3_5", "res3_6"):
        x = triple("mres", res_block(n), x, tiling((16, 20), (8, 10), small_batch(N, H // 8, W // 8, 16, 20, n_cu)), out=n)
    x = triple("mres", ("conv3_5", "conv3_6", "conv4_1"), x, tiling((8, 10), (8, 4), small_batch(N, H // 16, W // 16, 8, 10, n_cu)))

    def chain(names, x, th, tw, stride, post=None, unchain=False, esplit=False):
        """mres_can_chain: the residual blocks of one shape run as ONE launch where the frame fits the tile."""
        h, w = H // stride, W // stride
        groups = [names] if h <= th and w <= tw else [[n] for n in names]
        for g in groups:
            last = g is groups[-1]
            layers = tuple(l for n in g for l in res_block(n)) + ((post,) if post and last else ())
            out = post if post and last else g[-1]
            kind, disp, tiles, form = "mres", 1, ((th, tw),), ""
            if len(g) > 1:
                if unchain and not F16 and small_batch(N, h, w, 16, 20, n_cu):     # launch_mres: not DT_F16, scratch tensor, no post conv
                    kind, disp, tiles, form = "mres.unchained", len(g), ((8, 10),), "block by block on 8x10 tiles"
                elif esplit and F32 and split_sums and (h, w) == (8, 10) and N <= ESPLIT_MAX_FRAMES:
                    kind, disp, form = "mres.esplit", len(g) + 1, "mres_esplit_kernel"
                else:
                    kind, form = "mres.chain", "one launch"
            if post and last:
                kind += ".post"
            add(kind, layers, [x], [out], k_mres([res_block(n) for n in g], True, post=post if last else None), blocks=g, tiles=tiles,
                dispatches=disp, form=form, fp32_layers=(post,))
            x = out
        return x

    x = chain(["res4_1", "res4_2", "res4_3", "res4_4"], x, 16, 20, 16, unchain=True)
    h32, w32 = H // 32, W // 32
    tl, fm = tiling((8, 10), (8, 4), small_batch(N, h32, w32, 8, 10, n_cu))
    add("mres.wexp", ("conv4_2", "conv4_3", "conv5_1"), [x], ["conv5_1", "conv4_2"], k_mres([("conv4_2", "conv4_3", "conv5_1")], False, wexp=True),
        tiles=tl, form=fm)
    x = chain(["res5_1", "res5_2", "res5_3", "res5_4", "res5_5"], "conv5_1", 8, 10, 32, post="conv5_2" if deep else None, esplit=True)
    if not deep:
        add("pw", ("conv5_2",), [x], ["conv5_2"], k_layer("conv5_2", False, gemm=True))
    tl = ((16, 20), (8, 10)) if F16 else ((8, 10),)                    # the stride-32 mdw pair: fp32 storage always on 8x10 tiles
    if deep and h32 <= 8 and w32 <= 10 and num_out <= 32:              # mdw2_can_chain: tile == frame and one pair of head tiles
        es = F32 and split_sums and (h32, w32) == (8, 10) and N <= ESPLIT_MAX_FRAMES       # mdw2_esplit_ok (its headn <= 32 holds here)
        add("mdw2.esplit" if es else "mdw2", ("conv5_3", "conv5_4", "conv5_5", "conv5_6", "head_5"), ["conv5_2"], ["head_small"],
            k_mdw([("conv5_3", "conv5_4"), ("conv5_5", "conv5_6")], "head_5"), tiles=((8, 10),), dispatches=3 if es else 1,
            form="mdw2_esplit_kernel" if es else "one launch", keep_form=head_forms)
    else:
        # YF_MDW_SHAPES has the 128-channel pair on 8x10 tiles only, in every dtype (the fp16 table lists 16x20 too, as it always has)
        add("mdw", ("conv5_3", "conv5_4"), ["conv5_2"], ["conv5_4"], k_mdw([("conv5_3", "conv5_4")], None), tiles=tl,
            form="8x10 HM0" if head_forms else "", keep_form=head_forms)
        add("mdw.head", ("conv5_5", "conv5_6", "head_5"), ["conv5_4"], ["head_small"], k_mdw([("conv5_5", "conv5_6")], "head_5"), tiles=tl,
            form="8x10 HM%d" % HM if head_forms else "", keep_form=head_forms)
    if deep:
        few = 2 * N * (-(-(h32 * w32) // 80)) <= n_cu
        add("dcat", ("deconv5_1", "conv4_1_1"), ["conv5_2", "conv4_2"], ["conv4_1_1"], k_dcat(),
            form="one M-tile per item" if few else "five M-tiles per item")
    else:
        add("pw", ("deconv5_1",), ["conv5_2"], ["deconv5_1"], k_layer("deconv5_1", False, gemm=True))
        add("pw", ("conv4_1_1",), ["conv4_2", "deconv5_1"], ["conv4_1_1"], k_layer("conv4_1_1", False, gemm=True))
    h16 = H // 16
    few16 = h16 > 8 and small_batch(N, h16, W // 16, 16, 20, n_cu)                                # launch_mdw: `a.H > 8 && 2 * big_tiles <= n_cu`
    tl, fm = tiling((16, 20), (8, 10), few16)
    fm0 = fmh = fm
    if head_forms:                                                      # ... whatever the dtype: the chosen tile, and the head mode beside it
        tl = ((8, 10),) if few16 else ((16, 20),)
        fm0, fmh = "%dx%d HM0" % tl[0], "%dx%d HM%d" % (tl[0] + (HM,))
    add("mdw", ("conv4_1_2", "conv4_1_3"), ["conv4_1_1"], ["conv4_1_3"], k_mdw([("conv4_1_2", "conv4_1_3")], None), tiles=tl, form=fm0,
        keep_form=head_forms)
    add("mdw.head", ("conv4_1_4", "conv4_1_5", "head_4"), ["conv4_1_3"], ["head_large"], k_mdw([("conv4_1_4", "conv4_1_5")], "head_4"), tiles=tl,
        form=fmh, keep_form=head_forms)
    return T


KINDS_F16 = ("valu", "k19h", "mres", "mres.wexp", "mres.chain", "mres.post", "mres.chain.post", "pw", "dcat", "mdw", "mdw.head", "mdw2")


def forms(table) -> Dict[str, Tuple[str, int, str]]:
    """{op name: (kind, dispatches, form)}: what each case asserts it reaches."""
    return {L.name: (L.kind, L.dispatches, L.form) for L in table}


def forms_text(table):
    return "\n".join("  %-16s x%d  dtype %d  %-28s %s" % (L.kind, L.dispatches, L.dtype, L.form, L.name[:60]) for L in table)


# ---- running -----------------------------------------------------------------------------------------------------------------------------

def run_ctx(launch, net, inputs, precision, mode):
    """One launch from the given input tensors (dict name -> tensor, any float dtype) -> ({name: output}, the context it ran in)."""
    c = Ctx(net, precision, mode, bound=launch.kind in PROPAGATED_CAP)
    with torch.no_grad():
        outs = launch.fn(c, tuple(inputs[n].to(c.dtype) for n in launch.inputs))
    return dict(zip(launch.outputs, outs)), c


def run(launch, net, inputs, precision, mode="twin"):
    return run_ctx(launch, net, inputs, precision, mode)[0]


def chained(table, net, x, precision, mode="twin"):
    """All launches in order, each from its predecessors' outputs -> every tensor of the plan."""
    t = {"input": x}
    for L in table:
        t.update(run(L, net, t, precision, mode))
    return t


def collect(yf, m, table, xd, launches=None):
    """GPU side: the engine's [(op name, dtype handed to the kernel, dispatches)] for the model's present fusion / precision, and {name:
    tensor on the CPU} of the input, the heads of one forward and every tensor of the table that exists in device memory (`model.probe`).
    The engine's ops and the table's entries are the same list, one to one, and a tensor that a launch keeps on chip is not skipped silently:
    it reports YF_E_NOPROBE, and its launch is replayed as one unit.  launches: the entries of the table whose tensors are wanted (default: all);
    the op list is held to the WHOLE table either way."""
    import pytest
    e = m.engine(xd.shape[2], xd.shape[3], xd.shape[0], xd.device)
    n = ctypes.c_int()
    yf._lib.check(e.lib.yf_num_launches(e.handle, ctypes.byref(n)))
    ops = []
    for i in range(n.value):
        buf = ctypes.create_string_buffer(512)
        b, fm, fv, kdt, nd = ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_int(), ctypes.c_int()
        yf._lib.check(e.lib.yf_op_info_ex(e.handle, i, buf, 512, ctypes.byref(b), ctypes.byref(fm), ctypes.byref(fv)))
        yf._lib.check(e.lib.yf_op_dtype(e.handle, i, ctypes.byref(kdt)))
        yf._lib.check(e.lib.yf_op_dispatches(e.handle, i, xd.shape[0], ctypes.byref(nd)))
        ops.append((buf.value.decode(), kdt.value, nd.value))
    assert [o[0] for o in ops] == [L.name for L in table], ([o[0] for o in ops], [L.name for L in table])
    with torch.no_grad():
        hl, hs = m(xd)
    tensors = {"input": xd.cpu(), "head_large": hl.cpu(), "head_small": hs.cpu()}
    for L in (table if launches is None else launches):
        for name in L.inputs + L.outputs:
            if name not in tensors:
                tensors[name] = m.probe(xd, name).cpu()
        for name in L.internal:
            with pytest.raises(yf._lib.YFError, match="error -5"):
                m.probe(xd, name)
    return ops, tensors


# ---- the comparators ---------------------------------------------------------------------------------------------------------------------
#
# fp16 storage.  Two correct evaluations of a launch (another summation order in fp32) differ in three ways:
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
#
# fp32 storage.  Nothing is rounded inside a launch, so only 2. remains: the distance in fp32 ulps at max(|exact|, M), held to the margin
# times the twin's and to THE CAP (below).

def ulp16(a):
    """One fp16 ulp at |a| (float64 array), subnormals counted as the smallest normal's: 2^(floor(log2 max(|a|, 2^-14)) - 10)."""
    m = np.maximum(np.abs(a), 2.0 ** -14)
    return np.exp2(np.floor(np.log2(m)) - 10)


def ulp32(m):
    """One fp32 ulp at |m| (float64 array): 2^(floor(log2 m) - 23); subnormals counted as the smallest normal's."""
    return np.exp2(np.floor(np.log2(np.maximum(np.abs(m), 2.0 ** -126))) - 23)


def where(mark, dist, tiles, describe, top=5):
    """Which elements are marked and what they have in common: how many, the share on the border and on a tile seam, per frame, the busiest
    channel, the last row and column, and the `top` marked elements of largest `dist`, each as `describe(index)` says."""
    N, C, Hh, Ww = mark.shape
    idx = np.argwhere(mark)
    order = np.argsort(-dist[mark], kind="stable")[:top]
    n, ch, y, x = idx.T
    border = (y == 0) | (y == Hh - 1) | (x == 0) | (x == Ww - 1)
    seam = np.zeros(len(idx), bool)
    for th, tw in tiles:
        seam |= ((y % th == 0) | (y % th == th - 1)) & (Hh > th) | ((x % tw == 0) | (x % tw == tw - 1)) & (Ww > tw)
    worst = ["(n=%d, c=%d, y=%d, x=%d): %s%s%s" % (*idx[i], describe(tuple(idx[i])), ", border" if border[i] else "", ", tile seam" if seam[i] else "")
             for i in order]
    ring = 1.0 - max(Hh - 2, 0) * max(Ww - 2, 0) / float(Hh * Ww)
    return ("%d of %d elements; %.0f %% of them on the border rows / columns (%.0f %% of the tensor lie there), %.0f %% on a tile seam of %s; "
            "per frame %s; busiest channel %d with %d; last column %d, last row %d; worst: %s"
            % (len(idx), mark.size, 100 * border.mean(), 100 * ring, 100 * seam.mean(), list(tiles), np.bincount(n, minlength=N).tolist(),
               int(np.bincount(ch).argmax()), int(np.bincount(ch).max()), int((x == Ww - 1).sum()), int((y == Hh - 1).sum()), "; ".join(worst)))


@dataclasses.dataclass
class Cmp:
    share: float            # share of elements with got != rne16(exact64) (fp32 outputs: with |got - exact64| > 2e-5 max(1, max |exact64|))
    far: float              # share of elements further than half an fp16 ulp at the terms' size
    dist: float             # largest |got - exact64| in fp16 ulps at max(|exact64|, terms' size)
    ulps: float             # largest |got - exact64| in fp16 ulps of max(|exact64|, 2^-14): reported only
    n_diff: int
    where: str              # the worst offenders and what they have in common


def compare(got, exact64, scale64=None, tiles=(), fp32=False, far_only=False, top=5) -> Cmp:
    """The fp16 criterion's figures of one tensor."""
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
        c.where = where(mark, dist, tiles, lambda i: "got %.6g, exact %.6g" % (g[i], e[i]), top)
    return c


def by_distance(launch):
    """fp16 launches whose "differs" is "further than half an fp16 ulp at the terms' size": the chains (see above) and the two head launches.
    The heads are fp32, but their operand is rounded to fp16 inside the launch (A); where that rounding falls the other way a logit moves by
    up to 2^-10 of one term, which is outside the fp32 criterion (2e-5 of the logits' range) whenever a term exceeds 2 % of the range: 2.4 %
    of the small head's logits with the seeded random weights, twin against float64.  The share outside the fp32 criterion is held to the
    margin times the twin's own as a third criterion (F32_REFERENCE_F16), without the 2 % cap, which the twin itself exceeds there."""
    return ".chain" in launch.kind or launch.fp32_out


def limits(kind, reference):
    """The fp16 criteria of one launch kind from the reference-against-itself figures (share, distance) of that kind: the margin times the
    share and never more than 2 %; the distance + 1 ulp and never more than 8."""
    share, dist = reference[kind]
    return min(MARGIN * share, SHARE_CAP), min(dist + 1.0, ULP_CAP)


def verdict(launch, out_name, c: Cmp, reference, f32_reference=None):
    """None if the tensor passes the fp16 criteria, else the assertion text: which launch, which tensor, where."""
    smax, dmax = limits(launch.kind, reference)
    share = c.far if by_distance(launch) else c.share
    f32max = MARGIN * (f32_reference or F32_REFERENCE_F16)[launch.kind] if launch.fp32_out else 1.0
    if share <= smax and c.dist <= dmax and (not launch.fp32_out or c.share <= f32max):
        return None
    what = "are further than half an fp16 ulp (at the size of the summed terms) from the exact value" if by_distance(launch) else "differ from rne16(exact)"
    if launch.fp32_out:
        what += " and %.3f %% are further than 2e-5 of the range (limit %.3f %%)" % (100 * c.share, 100 * f32max)
    return ("launch %s [%s] -> %s: %.3f %% of the elements %s (limit %.3f %%), largest distance %.2f fp16 ulps at the terms' size (limit %.2f; "
            "%.0f in the result's own ulps); %s" % (launch.name, launch.kind, out_name, 100 * share, what, 100 * smax, c.dist, dmax, c.ulps, c.where))


@dataclasses.dataclass
class Dist:
    dist: float          # largest |got - exact| in fp32 ulps at max(|exact|, M)
    own: float           # ... in the result's own fp32 ulps (results below 2^-20 counted as 2^-20): reported only
    where: str           # the elements past the limit and what they have in common
    cap_used: float = 0.0   # largest |got - exact| as a share of the a-priori bound (the launch's cap)


def distance(got, exact64, scale64, tiles=(), limit=None, cap_ulps=None, bound64=None) -> Dist:
    """The fp32 criterion's figures of one tensor.  limit, cap_ulps: in fp32 ulps at the terms' size; bound64: the propagated bound per element
    (absolute), which replaces cap_ulps: an element is then held to min(limit ulps, its bound)."""
    g, e = got.detach().cpu().double().numpy(), exact64.detach().cpu().double().numpy()
    assert g.shape == e.shape, (g.shape, e.shape)
    assert bool(np.isfinite(g).all()), "a non-finite output"
    m = np.maximum(np.abs(e), scale64.detach().cpu().double().numpy())
    err = np.abs(g - e)
    d = err / ulp32(m)
    out = Dist(float(d.max()), float((err / ulp32(np.maximum(np.abs(e), 2.0 ** -20))).max()), "")
    if bound64 is not None:                     # the distance scaled per element so that `limit` is the criterion
        b = bound64.numpy() / ulp32(m)
        out.cap_used = float((d / b).max())
        if limit is not None:
            d = d * (limit / np.minimum(limit, b))
    elif cap_ulps:
        out.cap_used = out.dist / cap_ulps
    if limit is not None and float(d.max()) > limit:
        out.where = where(d > limit, d, tiles, lambda i: "got %.9g, exact %.9g, terms' size %.3g" % (g[i], e[i], m[i]))
    return out


# THE CAP.  A launch's limit may not exceed its a-priori forward-error bound: the sum, over the launch's layers, of the number of terms an
# output sums, in fp32 ulps at the terms' size (four times that for a split-operand GEMM) -- Launch.terms.  The twin stays inside it in
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
    """The fp32 GPU criterion of a launch: the margin times the twin's worst distance of its (precision, kind), never more than the cap."""
    ref = (reference or REFERENCE_F32)[(precision, launch.kind)]
    return MARGIN * ref if launch.kind in PROPAGATED_CAP else min(MARGIN * ref, cap(launch))


def replay_and_check(launch, net, tensors, got, precision, reference=None, f32_reference=None):
    """The float64 replay of one launch from `tensors` (its inputs) against `got` (its outputs), under the criterion of the precision.
    f16 -> [(out_name, Cmp, the share its kind is held to, verdict or None)]; f32, f16x3 -> [(out_name, Dist, verdict or None)].
    reference: another table than REFERENCE_F16 / REFERENCE_F32; f32_reference: ... than F32_REFERENCE_F16."""
    exact, c = run_ctx(launch, net, tensors, precision, "exact")
    res = []
    if precision == "f16":
        for i, (name, e) in enumerate(exact.items()):
            cm = compare(got[name], e, c.scale[i], launch.tiles, fp32=launch.fp32_out, far_only=by_distance(launch))
            res.append((name, cm, cm.far if by_distance(launch) else cm.share, verdict(launch, name, cm, reference or REFERENCE_F16, f32_reference)))
        return res
    lim = limit(precision, launch, reference)
    prop = launch.kind in PROPAGATED_CAP
    for i, (name, e) in enumerate(exact.items()):
        d = distance(got[name], e, c.scale[i], launch.tiles, lim, cap(launch), c.bound if prop else None)
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


# fp16: what the float32 twin differs from the float64 replay by, per launch kind: the worst share of differing elements (chains: of elements
# further than half an ulp at the terms' size; fp32 outputs: outside the fp32 criterion) and the largest distance, over the whole
# parametrisation of the GPU test.  tests/test_cpu_f16_replay.py::test_reference_against_itself measures them again, asserts that none is
# exceeded and that each is within the caps; the header table of that file has the figures as measured, beside the GPU's.
REFERENCE_F16: Dict[str, Tuple[float, float]] = {
    "valu": (0.0056, 1.0), "k19h": (0.00215, 1.0), "mres": (0.00274, 1.0), "mres.wexp": (0.00106, 1.0), "mres.chain": (0.00348, 1.82),
    "mres.post": (0.00119, 0.5), "mres.chain.post": (0.00035, 1.0), "pw": (0.00061, 1.0), "dcat": (0.00157, 0.5), "mdw": (0.0033, 1.0),
    "mdw.head": (0.0, 0.33), "mdw2": (0.0, 0.42),
}
F32_REFERENCE_F16: Dict[str, float] = {"mdw.head": 0.0132, "mdw2": 0.0238}   # the head launches: worst share of logits outside the fp32 criterion, twin against float64

# fp32 storage: the twin's worst distance from the float64 replay per (precision, launch kind), in fp32 ulps at the terms' size, over the
# whole parametrisation (CASES_F32 x weights): tests/test_cpu_plan_replay.py measures them again and asserts that none is exceeded; the GPU
# is held to MARGIN times these, and never to more than a launch's cap.
REFERENCE_F32: Dict[Tuple[str, str], float] = {
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


# ---- inputs and cases shared by the CPU and the GPU tests ----------------------------------------------------------------------------------

SIZES = ((96, 160), (160, 224), (256, 352))


def frames_u8(golden, H, W, N, seed=0):
    """Uniform-noise frames; frame 1 is a bundled test frame cropped to the size (realistic activation statistics)."""
    u8 = np.random.default_rng(1000 * H + W + seed).integers(0, 256, size=(N, H, W), dtype=np.uint8)
    big = golden("golden_512")["input_u8"][3]
    u8[1] = big[64:64 + H, 96:96 + W]
    return u8


def state_dicts():
    import os
    from tests.random_weights import random_state_dict
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    shipped = os.path.join(root, "yolo-fastest-and-embedded-deployment_amd", "assets", "weights", "yolo_fastest_256x320_epoch28.pth")
    return {"shipped": lambda: bo.load_state_dict(shipped), "random": lambda: random_state_dict(0)}


# fp16 storage, (H, W, N): partial tiles everywhere; the stride-16 / 32 frames fit one tile; one column of tiles more than the chains allow.
# Batches: 2 takes every launcher's few-frames tiling; the large one takes the many-frames tiling -- the launchers switch at 2 N tiles <= #CU
# (256 CUs; mres_small_batch and its likes), i.e. above 128 frames where a frame is one tile and above 32 where it is four.  (The split-sum
# launches and launch_mres's block-by-block form, which switch at 9 frames, do not exist for fp16 storage.)
CASES_F16 = ((96, 160, 2), (96, 160, 132), (160, 224, 2), (160, 224, 36), (256, 352, 2))

# fp32 storage, (H, W, N, fusion levels, precisions): tests/test_gpu_plan_replay.py's parametrisation; what each reaches is asserted by `expect`
CASES_F32 = (
    (96, 160, 2, (1, 2), FP32_STORAGE),
    (96, 160, 132, (1, 2), FP32_STORAGE),
    (160, 224, 2, (1, 2), FP32_STORAGE),
    (160, 224, 36, (1, 2), FP32_STORAGE),
    (256, 352, 2, (1, 2), FP32_STORAGE),
    (256, 320, 2, (1, 2), ("f32",)),
    (256, 320, ESPLIT_MAX_FRAMES, (1, 2), ("f32",)),
    (256, 320, ESPLIT_MAX_FRAMES + 1, (1, 2), ("f32",)),
    (96, 160, 2, (0,), FP32_STORAGE),
    (160, 224, 36, (0,), FP32_STORAGE),
)
RANDOM_ONLY = {(96, 160, 132), (160, 224, 36)}        # fp32 storage: the large batches run with the seeded random weights only (a few seconds per test)

RES4 = "+".join(l for n in ("res4_1", "res4_2", "res4_3", "res4_4") for l in res_block(n))
RES5 = "+".join(l for n in ("res5_1", "res5_2", "res5_3", "res5_4", "res5_5") for l in res_block(n))
MDW2 = "conv5_3+conv5_4+conv5_5+conv5_6+head_5"


def expect(H, W, N, fusion, precision, n_cu):
    """{op name: (kind, dispatches)} a CASES_F32 case exists for, for a device of n_cu compute units (256 on an MI355X)."""
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
            e["+".join(res_block(n))] = ("mres", 1)
        e["conv5_3+conv5_4"] = ("mdw", 1)
        e["conv5_5+conv5_6+head_5"] = ("mdw.head", 1)
    if (H, W) == (256, 320):
        es = precision == "f32" and N <= ESPLIT_MAX_FRAMES
        e[RES4] = ("mres.unchained", 4) if few else ("mres.chain", 1)
        e[RES5 + post] = ("mres.esplit" + p, 6) if es else ("mres.chain" + p, 1)
        if fusion == 2:
            e[MDW2] = ("mdw2.esplit", 3) if es else ("mdw2", 1)
    return e


# ---- the io-dependent launches at other io_params (tests/test_cpu_io_replay.py, tests/test_gpu_io_replay.py) ------------------------------
#
# Three kinds of launch depend on io_params: the stem through input_channel (with conv0 as a launch of its own, and the pre = false block
# behind it, above four planes), the two head launches through num_out.  Only these are replayed here, from the tensors the device (or the
# twin) produced, at the configurations of tests/io_cfg.py, in every tile form the launchers have for them.
# case -> (sizes, N (None: n_cu // 8 + 1, the first batch at which four 16x20 tiles per frame leave the few-frames rule), configurations,
#          precisions, fusion levels)
IO_ALL = ("c1", "c5rgb", "c20", "a2", "c80rgb", "ch2", "ch4", "ch6")
IO_CASES = {
    "few": (((256, 320),), 2, IO_ALL, PRECISIONS, (1, 2)),
    "layers": (((256, 320), (96, 160)), 2, ("c1", "c5rgb", "c80rgb", "ch4", "ch6"), FP32_STORAGE, (0,)),
    "chain": (((256, 320),), ESPLIT_MAX_FRAMES + 1, ("c1", "a2", "c5rgb"), ("f32",), (2,)),
    "low": (((96, 160),), 2, ("c1", "a2", "c5rgb", "c20", "c80rgb", "ch2"), PRECISIONS, (2,)),
    "many": (((288, 352),), None, ("a2", "c1", "c5rgb", "c20", "c80rgb", "ch6"), PRECISIONS, (1, 2)),
}
STEM, STEM_BLOCK = "conv0+conv1_2+conv1_3+conv1_4", "conv1_2+conv1_3+conv1_4"
HEAD_L, HEAD_S = "conv4_1_4+conv4_1_5+head_4", "conv5_5+conv5_6+head_5"


def io_params_list():
    """[(case, H, W, N or None, tag, precision, fusion)]: the parametrisation of both io replay tests."""
    return [(c, H, W, N, t, p, f) for c, (sizes, N, tags, precs, fus) in IO_CASES.items() for H, W in sizes for t in tags for p in precs for f in fus]


def io_batch(N, n_cu):
    return n_cu // 8 + 1 if N is None else N


def io_launches(table):
    """The launches of a table that depend on io_params."""
    return [L for L in table if L.name == STEM_BLOCK or {"conv0", "head_5", "head_4"} & set(L.name.split("+"))]


def io_expect(case, H, W, N, fusion, precision, num_out, input_channel):
    """{op name: (kind, dispatches, form)} an IO_CASES case exists for (form "": not stated), written from the case list, not from the table:
    the large head's tile and head mode, the small head's launch, the stem's."""
    hm = "HM%d" % (1 if num_out <= 32 else 2)
    e = {}
    if fusion == 0:
        return {"conv0": ("l.dense", 1, ""), "head_5": ("l.head", 1, ""), "head_4": ("l.head", 1, "")}
    if input_channel <= 4:
        e[STEM] = ("valu" if precision == "f16" else "valu.stem", 1, "")
    else:
        e["conv0"], e[STEM_BLOCK] = ("l.dense", 1, ""), ("valu", 1, "")
    e[HEAD_L] = ("mdw.head", 1, ("8x10 " if case in ("few", "chain") else "16x20 ") + hm)
    chainable = fusion == 2 and num_out <= 32 and H // 32 <= 8 and W // 32 <= 10
    if chainable and case in ("few", "chain"):
        es = precision == "f32" and N <= ESPLIT_MAX_FRAMES
        e[MDW2] = ("mdw2.esplit", 3, "mdw2_esplit_kernel") if es else ("mdw2", 1, "one launch")
    elif chainable:
        e[MDW2] = ("mdw2", 1, "one launch")
    else:
        e[HEAD_S] = ("mdw.head", 1, "8x10 " + hm)
    return e


# What the twin of an io-dependent launch differs from its float64 replay by WHERE a configuration exceeds the recorded figure of its kind
# (REFERENCE_F32 / REFERENCE_F16 / F32_REFERENCE_F16, which do not change): measured and asserted by tests/test_cpu_io_replay.py over
# IO_CASES, used by tests/test_gpu_io_replay.py for that configuration only.  The head conv's reduction length (96 or 128) does not depend on
# its width, so most configurations stay within the recorded figures of the shipped shape.
IO_REFERENCE_F32: Dict[Tuple[str, str, str], float] = {
    ("f32", "l.head", "c80rgb"): 6.08,             # 255 channels at fusion 0: 5.96 where the 24-channel head reaches 5.60
    ("f16x3", "l.head", "c80rgb"): 6.08,           # (the per-layer plan runs the same fp32 kernel in an f16x3 engine)
}
IO_REFERENCE_F16: Dict[Tuple[str, str], Tuple[float, float]] = {
    ("l.dense", "ch6"): (0.0004, 0.3),             # conv0 on its own with fp16 storage (conv0_any_kernel<half_t>): no shipped-shape figure exists
}
IO_F32_REFERENCE_F16: Dict[Tuple[str, str], float] = {    # share of fp32 logits outside 2e-5 of the range, twin against float64
    ("mdw.head", "c20"): 0.0145, ("mdw.head", "c80rgb"): 0.0187,
    ("mdw2", "a2"): 0.0455, ("mdw2", "c1"): 0.0294, ("mdw2", "c5rgb"): 0.0660,
}


def io_references(tag):
    """(REFERENCE_F32, REFERENCE_F16, F32_REFERENCE_F16) as configuration `tag` is held to them."""
    r32, r16, f16 = dict(REFERENCE_F32), dict(REFERENCE_F16), dict(F32_REFERENCE_F16)
    r32.update({(p, k): v for (p, k, t), v in IO_REFERENCE_F32.items() if t == tag})
    r16.update({k: v for (k, t), v in IO_REFERENCE_F16.items() if t == tag})
    f16.update({k: v for (k, t), v in IO_F32_REFERENCE_F16.items() if t == tag})
    return r32, r16, f16
