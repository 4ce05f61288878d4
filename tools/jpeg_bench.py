#!/usr/bin/env python3
"""Device JPEG decoder throughput (csrc/yf_jpeg_kernels.hip, jpeg.py).  GPU box:
    python tools/jpeg_bench.py --decode            event-timed device time of one decode call (memset + 3 kernels) for 256 bundled frames
                                                   (640x512 gray) and 256 generated 640x512 4:2:0 frames at quality 95; batch-1 latency;
                                                   end to end for 256 frames (file bytes in host memory -> BGR in HBM: pack + upload +
                                                   decode + status check) against PIL on one host thread
    python tools/jpeg_bench.py --decode --profile  the --decode run under `rocprofv3 --kernel-trace --stats` (a child process, a run of its
                                                   own): each kernel's share
    python tools/jpeg_bench.py --progressive       the same 256 + 256 frames re-saved by Pillow as progressive files (progressive=True): device time
                                                   of one call, batch-1 latency, end to end against PIL on one host thread on the same
                                                   files, and the device time of the baseline twins (the same re-save without
                                                   progressive), all in this run; with --profile each kernel's share
    python tools/jpeg_bench.py --train             train() examples/s at batch 16 (DataLoader + train_step), interleaved over --rounds:
                                                   cache=None decode="device", cache=None decode="host", cache="device\""""
import argparse
import csv
import glob
import io
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import yolo_fastest_amd as yf  # noqa: E402
from yolo_fastest_amd import jpeg, training, validation as val  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--decode", action="store_true")
ap.add_argument("--progressive", action="store_true")
ap.add_argument("--profile", action="store_true")
ap.add_argument("--train", action="store_true")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--out", default=None, help="directory for the rocprofv3 output (default: a new temporary directory)")
a = ap.parse_args()
dev = torch.device("cuda:0")
BUNDLED = os.path.join(ROOT, "tests", "golden", "test_data")


def bundled(n):
    files = [open(os.path.join(BUNDLED, f), "rb").read() for f in sorted(os.listdir(BUNDLED))]
    return (files * (n // len(files) + 1))[:n]


def color420(n):
    import jpeg_gen as jg
    rng = np.random.default_rng(0)
    out = []
    for i in range(n):
        a_ = jg.image("smooth", 640, 512, rng)
        a_ = np.clip(a_.astype(int) + rng.integers(-24, 25, a_.shape), 0, 255).astype(np.uint8)   # texture on gradients
        out.append(jg.encode(a_, "420", quality=95))
    return out


def resaved(datas, quality, **kw):
    """The files' pixels saved again by Pillow (mode kept)."""
    from PIL import Image
    import jpeg_gen as jg
    out = []
    for d in datas:
        b = io.BytesIO()
        with jg.big_encoder_buffer():
            Image.open(io.BytesIO(d)).save(b, "JPEG", quality=quality, **kw)
        out.append(b.getvalue())
    return out


def device_ms(datas, progressive=False):
    blob, h, w = jpeg.pack(datas, progressive=progressive)
    d_blob = torch.empty(blob.numel(), dtype=torch.uint8, device=dev)
    d_blob.copy_(blob)
    ws = torch.empty(jpeg.workspace_bytes(blob), dtype=torch.uint8, device=dev)
    out = torch.empty((len(datas), h, w, 3), dtype=torch.uint8, device=dev)
    st = torch.empty((len(datas),), dtype=torch.int32, device=dev)
    from yolo_fastest_amd import _lib
    import ctypes
    lib = _lib.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream

    def call():
        _lib.check(lib.yf_jpeg_decode_u8(dev.index, ctypes.c_void_p(blob.data_ptr()), ctypes.c_void_p(d_blob.data_ptr()),
                                         ctypes.c_void_p(ws.data_ptr()), ws.numel(), ctypes.c_void_p(out.data_ptr()),
                                         ctypes.c_void_p(st.data_ptr()), ctypes.c_void_p(stream)))
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    assert not st.cpu().numpy().any()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / a.reps


def end_to_end(datas, progressive=False):
    from PIL import Image
    for _ in range(2):
        jpeg.decode_files(datas, dev, progressive=progressive)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(3):
        jpeg.decode_files(datas, dev, progressive=progressive)
    torch.cuda.synchronize()
    dev_ms = (time.perf_counter() - t) / 3 * 1e3
    t = time.perf_counter()
    for d in datas:
        np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(d)).convert("RGB"))[:, :, ::-1])
    pil_ms = (time.perf_counter() - t) * 1e3
    return dev_ms, pil_ms


def decode_bench():
    res = {}
    g, c = bundled(256), color420(256)
    for name, datas in (("gray640x512", g), ("yuv420_640x512_q95", c)):
        ms = device_ms(datas)
        one = device_ms(datas[:1])
        res[name] = {"device_ms_256": round(ms, 4), "frames_per_s_256": round(256 / ms * 1e3), "device_ms_1": round(one, 4),
                     "mean_file_bytes": int(np.mean([len(d) for d in datas]))}
        print("%s: 256 frames %.4f ms (%.0f frames/s); batch 1 %.4f ms; mean file %d B"
              % (name, ms, 256 / ms * 1e3, one, res[name]["mean_file_bytes"]))
    for name, datas in (("gray640x512", g), ("yuv420_640x512_q95", c)):
        dms, pms = end_to_end(datas)
        res[name].update(end_to_end_ms_256=round(dms, 2), pil_one_thread_ms_256=round(pms, 2))
        print("%s end to end, 256 files from host bytes: device path %.2f ms, PIL one thread %.2f ms (%.1fx)" % (name, dms, pms, pms / dms))
    return res


def progressive_bench():
    res = {}
    for name, src, q in (("gray640x512", bundled(20), 90), ("yuv420_640x512_q95", color420(256), 95)):
        prog = (resaved(src, q, progressive=True) * 13)[:256]
        twin = (resaved(src, q) * 13)[:256]
        assert all(b"\xff\xc2" in d[:1024] for d in prog) and not any(b"\xff\xc2" in d[:1024] for d in twin)
        ms, one = device_ms(prog, True), device_ms(prog[:1], True)
        tms, tone = device_ms(twin, True), device_ms(twin[:1], True)
        dms, pms = end_to_end(prog, True)
        res[name] = {"device_ms_256": round(ms, 4), "device_ms_1": round(one, 4), "twin_device_ms_256": round(tms, 4),
                     "twin_device_ms_1": round(tone, 4), "end_to_end_ms_256": round(dms, 2), "pil_one_thread_ms_256": round(pms, 2),
                     "mean_file_bytes": int(np.mean([len(d) for d in prog])), "twin_mean_file_bytes": int(np.mean([len(d) for d in twin]))}
        print("progressive %s: 256 frames %.4f ms (%.0f frames/s), baseline twins %.4f ms (%.1fx); batch 1 %.4f ms, twin %.4f ms; "
              "end to end %.2f ms, PIL one thread %.2f ms (%.2fx); mean file %d B, twin %d B"
              % (name, ms, 256 / ms * 1e3, tms, ms / tms, one, tone, dms, pms, pms / dms, res[name]["mean_file_bytes"],
                 res[name]["twin_mean_file_bytes"]))
    return res


def profile():
    out = a.out or tempfile.mkdtemp(prefix="jpeg_bench_")
    os.makedirs(out, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "jpeg", "--", sys.executable,
           os.path.abspath(__file__), "--progressive" if a.progressive else "--decode", "--reps", str(a.reps)]
    subprocess.check_call(cmd)
    for f in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
        with open(f) as fh:
            for row in csv.DictReader(fh):
                if "jpeg_" in row.get("Name", ""):
                    print("rocprofv3 %s: calls %s, average %.4f ms, min %.4f ms, max %.4f ms, share %s %%" % (
                        row["Name"][:40], row.get("Calls"), float(row.get("AverageNs", 0)) / 1e6, float(row.get("MinNs", 0)) / 1e6,
                        float(row.get("MaxNs", 0)) / 1e6, row.get("Percentage")))


def train_bench():
    from torch.utils.data import DataLoader
    from yolo_fastest_amd.dataset import DetectDataset
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    io_ = yf.io_params_for(256)
    torch.manual_seed(0)
    m = yf.YoloFastest(io_)
    m.initialize_weights()
    m = m.to(dev).train()
    crit = [val.YOLOLossV3(io_["anchors"][i], 3, io_["input_shape"], dev, model=m) for i in range(2)]
    opt = training.Adam(m.parameters(), lr=0.001)
    B = 16
    import voc_tree
    tmp = tempfile.mkdtemp()
    d = os.path.join(tmp, "train")
    os.makedirs(os.path.join(d, "img"))
    os.makedirs(os.path.join(d, "xml"))
    for c in range(13):                 # the 20 bundled frames with their fixture XMLs, linked 13 times: 260 items
        for s in voc_tree.bundled_stems():
            os.symlink(os.path.join(voc_tree.BUNDLED, s + ".jpg"), os.path.join(d, "img", "%s_%d.jpg" % (s, c)))
            os.symlink(os.path.join(voc_tree.VOC, "xml", s + ".xml"), os.path.join(d, "xml", "%s_%d.xml" % (s, c)))
    aug = dict(yf.config_params["augment_params"], train_dataset_dir=d, val_dataset_dir=d)
    setups = {"cache=None decode=device": dict(cache=None, decode="device"), "cache=None decode=host": dict(cache=None, decode="host"),
              "cache=device": dict(cache="device")}
    loaders = {n: DataLoader(DetectDataset(io_["input_shape"], io_["origin_img_shape"], None, aug_params=aug, device=dev, **kw), batch_size=B,
                             num_workers=0, drop_last=True, pin_memory=True, shuffle=True, collate_fn=val.collate_fn) for n, kw in setups.items()}

    def batches(name):
        while True:
            for imgs, targets in loaders[name]:
                yield imgs.to(dev).float(), targets.to(dev).float()
    gens = {n: batches(n) for n in setups}
    for n, g in gens.items():
        for _ in range(20):
            imgs, targets = next(g)
            training.train_step(m, crit, opt, imgs, targets)
    torch.cuda.synchronize()
    res = {n: [] for n in gens}
    for r in range(a.rounds):
        for n, g in gens.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(a.steps):
                imgs, targets = next(g)
                training.train_step(m, crit, opt, imgs, targets)
            torch.cuda.synchronize()
            res[n].append(B * a.steps / (time.perf_counter() - t))
    for n, v in res.items():
        print("train batch %d, %s: %.0f examples/s (median of %d rounds: %s)" % (B, n, float(np.median(v)), len(v), ["%.0f" % x for x in v]))
    ratio = np.median(res["cache=None decode=device"]) / np.median(res["cache=None decode=host"])
    print("decode=device / decode=host (cache=None) = %.2f" % ratio)
    return {n: float(np.median(v)) for n, v in res.items()}


out = {}
if (a.decode or a.progressive) and a.profile:
    profile()
elif a.progressive:
    out["progressive"] = progressive_bench()
elif a.decode:
    out["decode"] = decode_bench()
if a.train:
    out["train"] = train_bench()
if out:
    print(json.dumps(out))
