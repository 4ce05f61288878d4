"""TEST INFRASTRUCTURE (never imported by the product): CPU simulation of the rounding points of an fp16-storage evaluation of the
YoloFastest graph (yolo_fastest.py:150-218), used by tests/test_oracle_golden.py::test_fp16_rounding_alone_exceeds_the_surveys_tolerance
and tools/fp16_sim.py to show what SURVEY.md 8(d).3's "activations/weights fp16, fp32 accumulate" costs in logit error whoever
implements it.

Folded-BN forward in fp32 (torch CPU) with optional fp16 rounding of
  W  the pointwise / dense weights (MFMA operands),
  T  the tensors that live in HBM between launches of the fused plan (the narrow residual trunk + head-branch tensors),
  A  the activation operand of every pointwise MFMA (block input as the expansion's operand, depthwise result as the
     projection's operand),
  E  the expanded tensor kept on chip between expansion and the conv that consumes it -- WHERE THE KERNEL ROUNDS IT: conv1_8's result
     inside k19h_kernel (ReLU + RNE = the fp16 operand of conv1_9's MFMAs).  The MFMA block kernels (mres_kernel / mres_pc_kernel) keep
     E in LDS as float: their depthwise reads the un-rounded expansion, also conv4_3 (conv4_2 is rounded only on its way to HBM).

T depends on the plan, because a tensor is rounded where it is STORED (tests/replay.py lists every launch's rounding points with the
kernel line of each; tests/test_cpu_f16_replay.py holds this class bitwise to that launch-by-launch model):
  size=(H, W)  frames whose stride-16 / stride-32 maps fit one tile (16x20 / 8x10: mres_can_chain) run res4_1..4 / res5_1..5 as ONE launch
               each; a block's result stays in LDS as float, the next expansion rounds its operand (A), the residual adds the un-rounded
               value.  None: no chains (any larger frame, 640x512 among them).
  fusion=2     conv5_2 rides in the last res5 launch on the un-rounded tile with fp32 weights (no W, no A); where the frame fits one
               8x10 tile the small head is one launch and conv5_4 stays in LDS un-rounded.  (deconv5_1 + conv4_1_1 as one launch rounds
               the deconv result in registers: the same values.)
"""
import torch
import torch.nn.functional as F

from oracle import backbone_oracle as bo


def fold(sd):
    out = {}
    for name, kind, cin, cout, k, s, relu in bo.LAYERS:
        w = sd[name + ".0.weight"].double()
        sc = sd[name + ".1.weight"].double() / torch.sqrt(sd[name + ".1.running_var"].double() + 1e-5)
        b = sd[name + ".1.bias"].double() - sd[name + ".1.running_mean"].double() * sc
        w = w * (sc[None, :, None, None] if kind == "dc" else sc[:, None, None, None])
        out[name] = (w.float(), b.float())
    for h in ("head_5", "head_4"):
        out[h] = (sd[h + ".weight"].float(), sd[h + ".bias"].float())
    return out


def q(t):
    return t.half().float()


class Sim:
    # layers of the VALU block kernels (fp32 weights through the scalar path, fp32 arithmetic): never W / A rounded
    VALU = ("conv0", "conv1_2", "conv1_3", "conv1_4", "res1_1.conv1", "res1_1.conv2", "res1_1.conv3", "res2_1.conv1", "res2_1.conv2",
            "res2_1.conv3", "res2_2.conv1", "res2_2.conv2", "res2_2.conv3")

    E_ROUNDED = ("conv1_8",)   # expanded tensors a kernel rounds on chip (k19h_kernel); every other one stays fp32 in LDS

    def __init__(self, fw, W=False, T=False, A=False, E=False, split_w=False, split_a=False, valu_exact=True, size=None, fusion=1):
        self.fw, self.W, self.T, self.A, self.E, self.split_w, self.split_a = fw, W, T, A, E, split_w, split_a
        self.valu_exact = valu_exact
        H, Wd = size if size else (1 << 30, 1 << 30)
        self.chain4 = H // 16 <= 16 and Wd // 16 <= 20       # yf_mres_kernels.hip YF_MRES_SHAPES: res4 tile 16x20, res5 tile 8x10
        self.chain5 = H // 32 <= 8 and Wd // 32 <= 10
        self.deep = fusion >= 2

    def unit(self, name, x, store=False, is_exp=False, exact=False):
        _, kind, cin, cout, k, s, relu = bo._BY_NAME[name]
        w, b = self.fw[name]
        mfma = kind in ("c", "dc") and not (self.valu_exact and name in self.VALU) and not exact
        if mfma:
            if self.W and not self.split_w:
                w = q(w)
            if self.A and not self.split_a:
                x = q(x)
        if kind == "dc":
            y = F.conv_transpose2d(x, w, b, stride=2)
        else:
            y = F.conv2d(x, w, b, stride=s, padding=(k - 1) // 2, groups=(cin if kind == "dw" else 1))
        if relu:
            y = F.relu(y)
        if is_exp and self.E and name in self.E_ROUNDED:
            y = q(y)
        if store and self.T:
            y = q(y)
        return y

    def block(self, a, b, c, x, res, store=True):
        y = self.unit(a, x, is_exp=True)
        y = self.unit(b, y)
        y = self.unit(c, y)
        if res:
            y = y + x
        return q(y) if self.T and store else y

    def head(self, name, x):
        w, b = self.fw[name]
        if self.W and not self.split_w:
            w = q(w)
        if self.A and not self.split_a:
            x = q(x)
        return F.conv2d(x, w, b)

    def forward(self, x):
        with torch.no_grad():
            x = self.unit("conv0", x)
            x = self.block("conv1_2", "conv1_3", "conv1_4", x, False)
            x = self.block("res1_1.conv1", "res1_1.conv2", "res1_1.conv3", x, True)
            x = self.block("conv1_8", "conv1_9", "conv2_1", x, False)
            for n in ("res2_1", "res2_2"):
                x = self.block(n + ".conv1", n + ".conv2", n + ".conv3", x, True)
            x = self.block("conv2_2", "conv2_3", "conv3_1", x, False)
            for n in ("res3_1", "res3_2"):
                x = self.block(n + ".conv1", n + ".conv2", n + ".conv3", x, True)
            x = self.block("conv3_2", "conv3_3", "conv3_4", x, False)
            for n in ("res3_3", "res3_4", "res3_5", "res3_6"):
                x = self.block(n + ".conv1", n + ".conv2", n + ".conv3", x, True)
            x = self.block("conv3_5", "conv3_6", "conv4_1", x, False)
            for n in ("res4_1", "res4_2", "res4_3", "res4_4"):
                x = self.block(n + ".conv1", n + ".conv2", n + ".conv3", x, True, store=not self.chain4 or n == "res4_4")
            c42 = self.unit("conv4_2", x, is_exp=True)
            x = self.unit("conv4_3", c42)                     # the depthwise reads E from LDS, un-rounded ...
            if self.T:
                c42 = q(c42)                                  # ... the large head's concat reads conv4_2 from HBM
            x = self.unit("conv5_1", x, store=True)
            for n in ("res5_1", "res5_2", "res5_3", "res5_4", "res5_5"):
                x = self.block(n + ".conv1", n + ".conv2", n + ".conv3", x, True,
                               store=(not self.chain5 or n == "res5_5") and not (self.deep and n == "res5_5"))
            c52 = self.unit("conv5_2", x, store=True, exact=self.deep)
            x = self.unit("conv5_3", c52)
            x = self.unit("conv5_4", x, store=not (self.deep and self.chain5))
            x = self.unit("conv5_5", x)
            x = self.unit("conv5_6", x)
            hs = self.head("head_5", x)
            d = self.unit("deconv5_1", c52, store=True)
            x = self.unit("conv4_1_1", torch.cat((c42, d), 1), store=True)
            x = self.unit("conv4_1_2", x)
            x = self.unit("conv4_1_3", x, store=True)
            x = self.unit("conv4_1_4", x)
            x = self.unit("conv4_1_5", x)
            hl = self.head("head_4", x)
        return hl, hs
