#!/usr/bin/env python3
"""Training-step throughput (train.py:111-132: zero_grad, train-mode forward, two-head loss, backward, Adam) on synthetic frames.
GPU box: python tools/train_bench.py [--batch 16] [--steps 20] [--optimizer reference|adam|sgd] [--ema off|fused|loop] [--box-loss giou|diou|ciou] [--loss-hyp all] [--cpu]   (--cpu also times oracle/ on the host cores: the baseline)"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import yolo_fastest_amd as yf  # noqa: E402
from yolo_fastest_amd import training, validation as val  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=8)
ap.add_argument("--res", type=int, default=256)
ap.add_argument("--optimizer", choices=["reference", "adam", "sgd"], default="reference",
                help="reference: train.py:84's Adam on one group; adam / sgd: what training.train(optimizer=...) builds, three groups")
ap.add_argument("--branch-weight", type=float, nargs=2, default=None, metavar=("LARGE", "SMALL"),
                help="train_step(branch_weight=...): factors other than 1 take one backward per head")
ap.add_argument("--ema", choices=["off", "fused", "loop"], default="off",
                help="yolov5's ModelEMA behind every step: fused = training.ModelEMA inside the optimizer's launch (train_step(ema=...)); "
                     "loop = yolov5's own update(), a Python loop over the state dict on torch kernels")
ap.add_argument("--box-loss", choices=["giou", "diou", "ciou"], default=None, metavar="KIND",
                help="YOLOLossV3(box_loss=KIND): one IoU-family box term per positive cell in place of the reference's four (giou, diou, ciou)")
ap.add_argument("--loss-hyp", choices=["all"], default=None,
                help="all: every objectness / class option of YOLOLossV3 away from its neutral value (obj_pw 1.7, cls_pw 0.6, label_smoothing 0.1, "
                     "fl_gamma 1.5, fl_alpha 0.3, lambda_conf 0.7, lambda_cls 1.3, and obj_iou 1 when --box-loss is given): timing values, not a recipe")
ap.add_argument("--cpu", action="store_true")
ap.add_argument("--json", action="store_true", help="also print one JSON line (metric, value, ms per iteration, cpu baseline)")
a = ap.parse_args()
dev = torch.device("cuda:0")
io = yf.io_params_for(a.res)
H, W = io["input_shape"][0], io["input_shape"][1]
torch.manual_seed(0)
m = yf.YoloFastest(io)
m.initialize_weights()
sd0 = {k: v.clone() for k, v in m.state_dict().items()}
m = m.to(dev).train()
x = torch.rand(a.batch, 1, H, W) - 0.5
rng = np.random.default_rng(0)
t = np.zeros((a.batch, 64, 6), np.float32)
for b in range(a.batch):
    k = 1 + b % 6
    t[b, :k, 0:2] = rng.uniform(0.05, 0.95, (k, 2)); t[b, :k, 2:4] = rng.uniform(0.03, 0.4, (k, 2))
    t[b, :k, 4] = rng.integers(0, 3, k); t[b, :k, 5] = 255.0
tt = torch.from_numpy(t)
hyp = {}
if a.loss_hyp == "all":
    hyp = dict(obj_pw=1.7, cls_pw=0.6, label_smoothing=0.1, fl_gamma=1.5, fl_alpha=0.3, obj_iou=1.0 if a.box_loss else 0.0, lambda_conf=0.7,
               lambda_cls=1.3)
crit = [val.YOLOLossV3(io["anchors"][i], 3, io["input_shape"], dev, model=m, box_loss=a.box_loss, **hyp) for i in range(2)]
tp = yf.config_params["train_params"]
if a.optimizer == "reference":               # train.py:84: one group
    opt = training.Adam(m.parameters(), lr=0.001)
elif a.optimizer == "adam":                  # train(optimizer="adam"): yolov5's three groups, the decay on the convolution weights
    opt = training.Adam(training.param_groups(m, tp["weight_decay"]), lr=0.001, betas=(tp["momentum"], 0.999))
else:                                        # train(optimizer="sgd")
    opt = training.SGD(training.param_groups(m, tp["weight_decay"]), lr=0.001, momentum=tp["momentum"], nesterov=True)
xd, td = x.to(dev), tt.to(dev)
ema = training.ModelEMA(m) if a.ema != "off" else None


def loop_update():
    """yolov5's ModelEMA.update (utils/torch_utils.py), on the same EMA network"""
    ema.updates += 1
    d = ema.decay(ema.updates)
    msd = m.state_dict()
    with torch.no_grad():
        for k, v in ema.ema.state_dict().items():
            if v.dtype.is_floating_point:
                v *= d
                v += (1 - d) * msd[k].detach()


def iteration():
    if a.ema == "loop":
        out = training.train_step(m, crit, opt, xd, td, a.branch_weight)
        loop_update()
        return out
    return training.train_step(m, crit, opt, xd, td, a.branch_weight, ema=ema)


for _ in range(a.warmup):
    iteration()
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(a.steps):
    loss = iteration()[0]
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / a.steps
print("GPU  batch %d %dx%d: %.2f ms / iteration, %.0f examples/s, loss %.4f" % (a.batch, H, W, dt * 1e3, a.batch / dt, float(loss.detach())))
line = {"metric": "training_examples_per_second", "value": round(a.batch / dt, 1), "unit": "examples/s", "ms_per_iteration": round(dt * 1e3, 3),
        "steps": a.steps, "warmup": a.warmup, "dtype": "f32", "data": "synthetic",
        "config": {"workload": "train.py:111-132 iteration (zero_grad, train-mode forward, two-head loss, backward, Adam)", "batch": a.batch,
                   "input": [H, W], "optimizer": a.optimizer, "ema": a.ema, "box_loss": a.box_loss, "loss_hyp": a.loss_hyp}, "cpu_baseline": None}
if a.cpu:
    from oracle import backbone_oracle as bo, loss_oracle as lo
    sd = bo.training_state(sd0)
    keys = bo.parameter_keys(sd)
    params = [sd[k] for k in keys]
    copt = torch.optim.Adam(params, lr=0.001)
    n = 3
    t0 = time.perf_counter()
    for _ in range(n):
        copt.zero_grad()
        hl, hs = bo.forward(sd, x, train=True)
        total = sum(lo.loss_head(h, tt, io["anchors"][i], 3, io["input_shape"])[0] for i, h in enumerate((hl, hs)))
        total.backward()
        copt.step()
    dc = (time.perf_counter() - t0) / n
    print("CPU oracle (torch, %d threads): %.1f ms / iteration, %.1f examples/s" % (torch.get_num_threads(), dc * 1e3, a.batch / dc))
    line["cpu_baseline"] = {"value": round(a.batch / dc, 2), "unit": "examples/s", "cores": torch.get_num_threads(), "kind": "port",
                            "sample": "%d iterations of the same batch through oracle/backbone_oracle.py + loss_oracle.py + torch.optim.Adam" % n}
if a.json:
    import json
    print(json.dumps(line))
