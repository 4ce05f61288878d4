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
                                                   cache=None decode="device", cache=None decode="host", cache="device"
    python tools/jpeg_bench.py --encode            the result writer on the device (csrc/yf_jpeg_enc_kernels.hip): device time of one draw and of one
                                                   encode call for 256 frames (bundled 640x512, generated textured 640x512 and 480x640; quality 95,
                                                   4:2:0), batch-1 latency, end to end from device frames to bytes on the host against PIL on one
                                                   host thread on the same frames, the baseline decode time of the files PIL writes for those frames,
                                                   and batch_detect wall time per image over 256 files for the four combinations of decode and write,
                                                   --rounds interleaved rounds after one untimed round"""
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
ap.add_argument("--encode", action="store_true")
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


def timed(call, reps):
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def encode_bench():
    import logging
    import shutil
    from PIL import Image
    import jpeg_gen as jg
    from yolo_fastest_amd import plot
    res = {}
    rng = np.random.default_rng(0)

    def textured(w, h):
        out = []
        for _ in range(256):
            t = jg.image("smooth", w, h, rng)
            out.append(np.clip(t.astype(int) + rng.integers(-24, 25, t.shape), 0, 255).astype(np.uint8))
        return out
    sets = {"bundled640x512": [np.asarray(Image.open(io.BytesIO(d)).convert("RGB")) for d in bundled(256)],
            "textured640x512": textured(640, 512), "textured480x640": textured(480, 640)}
    for name, rgb in sets.items():
        h, w = rgb[0].shape[:2]
        frames = torch.from_numpy(np.stack(rgb)).to(dev)
        s = jpeg.enc_setup(h, w, 3, 95, "4:2:0")
        ws = torch.empty(jpeg.enc_workspace_bytes(s, 256), dtype=torch.uint8, device=dev)
        out_ = torch.empty((256, h * w * 3 + 1024), dtype=torch.uint8, device=dev)
        ln, st = torch.empty(256, dtype=torch.int32, device=dev), torch.empty(256, dtype=torch.int32, device=dev)
        enc = timed(lambda: jpeg.encode_batch(frames, order="rgb", setup=s, workspace=ws, out=out_, lengths=ln, status=st), a.reps)
        assert not st.cpu().numpy().any()
        one = timed(lambda: jpeg.encode_batch(frames[:1], order="rgb", setup=s, workspace=ws, out=out_[:1], lengths=ln[:1], status=st[:1]), a.reps)
        # four boxes with labels per frame (the bundled frames carry 0..3 detections), and the dense configuration: 260 per frame
        row = {}
        for tag, k in (("draw_ms_256_4_boxes", 4), ("draw_ms_256_260_boxes", 260)):
            boxes = [[[int(x), int(y), int(x) + 90, int(y) + 70] for x, y in zip(rng.integers(0, w - 90, k), rng.integers(30, h - 70, k))]
                     for _ in range(256)]
            labels = [["cloud %.2f" % (j % 101 / 100) for j in range(k)] for _ in range(256)]
            colors = [[[106, 90, 205]] * k for _ in range(256)]
            cache = {}
            scratch = frames.clone()
            t = time.perf_counter()
            plot.draw_boxes_device(scratch, boxes, labels, colors, 3, "rgb", cache)
            torch.cuda.synchronize()
            t = time.perf_counter()
            plot.draw_boxes_device(scratch, boxes, labels, colors, 3, "rgb", cache)
            torch.cuda.synchronize()
            row[tag.replace("draw_ms", "draw_call_wall_ms")] = round((time.perf_counter() - t) * 1e3, 3)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            plot.draw_boxes_device(scratch, boxes, labels, colors, 3, "rgb", cache)
            e1.record()
            torch.cuda.synchronize()
            row[tag] = round(e0.elapsed_time(e1), 4)     # includes the upload of the records: one call as the driver issues it
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(3):
            files = jpeg.encode_frames(frames, order="rgb")
        e2e = (time.perf_counter() - t) / 3 * 1e3
        t = time.perf_counter()
        pil = []
        for f in rgb:
            b = io.BytesIO()
            Image.fromarray(f).save(b, "JPEG", quality=95)
            pil.append(b.getvalue())
        pil_ms = (time.perf_counter() - t) * 1e3
        assert files == pil, "device bytes differ from PIL's"
        dec = device_ms(pil)
        row.update(encode_ms_256=round(enc, 4), frames_per_s_256=round(256 / enc * 1e3), encode_ms_1=round(one, 4), end_to_end_ms_256=round(e2e, 2),
                   pil_one_thread_ms_256=round(pil_ms, 2), decode_ms_256_same_files=round(dec, 4), encode_below_decode=bool(enc < dec),
                   mean_file_bytes=int(np.mean([len(d) for d in pil])))
        res[name] = row
        print(name, json.dumps(row))
        del frames, ws, out_
    # batch_detect over 256 files of 640x512, the four combinations, interleaved
    tmp = tempfile.mkdtemp(prefix="yf_encode_bench_")
    data, result = os.path.join(tmp, "data"), os.path.join(tmp, "result")
    os.makedirs(data)
    names = sorted(os.listdir(BUNDLED))
    for i in range(256):
        shutil.copy(os.path.join(BUNDLED, names[i % len(names)]), os.path.join(data, "%03d_%s" % (i, names[i % len(names)])))
    logger = logging.getLogger("jpeg-bench-encode")
    logger.setLevel(logging.WARNING)
    wpath = os.path.join(ROOT, "yolo-fastest-and-embedded-deployment_amd", "assets", "weights", "yolo_fastest_256x320_epoch28.pth")
    combos = [(d, w_) for d in ("device", "host") for w_ in ("device", "host")]
    dets = {c: yf.Detect_YOLO(dev, wpath, {"io_params": yf.io_params_for(256)}, logger, decode=c[0], write=c[1]) for c in combos}
    times = {c: [] for c in combos}
    for rnd in range(a.rounds + 1):
        for c in combos:
            shutil.rmtree(result, ignore_errors=True)
            os.makedirs(result)
            torch.cuda.synchronize()
            t = time.perf_counter()
            dets[c].batch_detect(data, result, batch_size=64, in_flight=2)
            torch.cuda.synchronize()
            if rnd:
                times[c].append((time.perf_counter() - t) / 256 * 1e3)
            assert len(os.listdir(result)) == 256
    shutil.rmtree(tmp, ignore_errors=True)
    bd = {"decode=%s,write=%s" % c: {"ms_per_image_rounds": [round(v, 4) for v in times[c]]} for c in combos}
    dd, dh = times[("device", "device")], times[("device", "host")]
    bd["claim"] = {"device_writer_slowest_ms": round(max(dd), 4), "host_writer_fastest_ms": round(min(dh), 4), "met": bool(max(dd) < min(dh)),
                   "ratio_host_over_device_medians": round(float(np.median(dh) / np.median(dd)), 2)}
    res["batch_detect_256_files_640x512_batch_64"] = bd
    print(json.dumps(bd))
    return res


out = {}
if a.encode:
    out["encode"] = encode_bench()
elif (a.decode or a.progressive) and a.profile:
    profile()
elif a.progressive:
    out["progressive"] = progressive_bench()
elif a.decode:
    out["decode"] = decode_bench()
if a.train:
    out["train"] = train_bench()
if out:
    print(json.dumps(out))
