#!/usr/bin/env python3
"""DetectDataset throughput (dataset.py, csrc/yf_aug_kernels.hip).  GPU box:
    python tools/dataset_bench.py --kernel            augment launch (640x512 BGR -> 256x320 gray, blur / flip drawn like the reference)
                                                      at batch 16 and 512: event-timed ms and required bytes/s (source + float32 output);
                                                      then the same frames with the geometric keys active (yf_augment_warp_u8: every
                                                      frame warped with a perspective draw, half of them flipped upside down)
    python tools/dataset_bench.py --kernel --profile  the same under `rocprofv3 --kernel-trace --stats` (a child process, a run of its own):
                                                      the kernel's own average duration from the stats file
    python tools/dataset_bench.py --train             train() iterations (DataLoader + train_step) at batch 16, examples/s, interleaved:
                                                      DetectDataset cache="device", decode="device", cache=None (decode="host"), the first
                                                      two again with the geometric keys active, and tools/train_bench.py's no-data loop
    python tools/dataset_bench.py --kernel --mixup    the mix call (yf_augment_mix_u8 over resized frames: every frame has a partner, both
                                                      warped with perspective draws) beside the warp call and the plain launch at batch 16
                                                      and 512, in interleaved rounds: median and spread of each
    python tools/dataset_bench.py --train --mixup     train() at batch 16, cache="device", geometric keys active: DetectDataset(mixup=True)
                                                      with mixup 0.5 and 0.0 beside the flag-unset data set and the no-data loop
    python tools/dataset_bench.py --kernel --mosaic   the mosaic call (yf_augment_mosaic_u8 over resized frames: every output a mosaic of
                                                      four frames under a perspective draw) beside the warp call and the plain launch at
                                                      batch 16 and 512, in interleaved rounds: median and spread of each
    python tools/dataset_bench.py --train --mosaic    train() at batch 16, cache="device", geometric keys active: DetectDataset(mosaic=True)
                                                      with mosaic 1.0 and 0.0 beside the flag-unset data set and the no-data loop
    python tools/dataset_bench.py --letterbox         DetectDataset(letterbox=True)'s launch against its yardsticks: 256 BGR frames into the
                                                      320 x 256 gray net, blur / flip drawn like the reference, HIP events around every
                                                      repeat, 30 repeats, the candidates interleaved in one process, on a ragged batch
                                                      (the 8 sizes of tools/cv_pre_bench.py --letterbox) and on a uniform 512 x 640 one:
                                                      (a) yf_augment_letterbox_u8, one call   (b) yf_cv_letterbox_u8 into a scratch, then
                                                      yf_augment_u8 on the same-size scratch, two launches   (c) the default squash path:
                                                      one yf_augment_u8 launch per source size plus an index_copy_ per size group"""
import argparse
import csv
import glob
import json
import os
import random
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import yolo_fastest_amd as yf  # noqa: E402
from yolo_fastest_amd import _lib, training, validation as val  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--kernel", action="store_true")
ap.add_argument("--profile", action="store_true")
ap.add_argument("--train", action="store_true")
ap.add_argument("--mixup", action="store_true", help="the mixup variant of --kernel / --train")
ap.add_argument("--mosaic", action="store_true", help="the mosaic variant of --kernel / --train")
ap.add_argument("--letterbox", action="store_true", help="yf_augment_letterbox_u8 against its two-launch and squash yardsticks")
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--out", default=None, help="directory for the rocprofv3 output (default: a new temporary directory)")
a = ap.parse_args()
dev = torch.device("cuda:0")
GEOMETRIC = dict(degrees=10.0, translate=0.1, scale=1.5, shear=2.0, perspective=0.0005, flipud=0.5)   # yolov5-sized ranges


def kernel_bench():
    lib = _lib.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    res = {}
    for N in (16, 512):
        src = torch.randint(0, 256, (N, 512, 640, 3), dtype=torch.uint8, device=dev)
        rng = random.Random(0)
        prm = []
        for _ in range(N):        # the reference's draws at its default probabilities (gussian_filter 0.3, fliplr 0.5)
            k = (7 if rng.random() < 0.4 else 3) if rng.random() < 0.3 else 0
            prm.append(k | (int(rng.random() < 0.5) << 8))
        d_prm = torch.tensor(prm, dtype=torch.int32, device=dev)
        x = torch.empty((N, 1, 256, 320), dtype=torch.float32, device=dev)

        def launch():
            _lib.check(lib.yf_augment_u8(dev.index, src.data_ptr(), 512, 640, 3, None, N, N, None, None, 256, 320, 1, 15, d_prm.data_ptr(),
                                         None, x.data_ptr(), stream))
        for _ in range(5):
            launch()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.reps):
            launch()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / a.reps
        need = N * (512 * 640 * 3 + 256 * 320 * 4)
        res[N] = {"ms": round(ms, 4), "required_bytes": need, "TB_per_s": round(need / ms / 1e9, 3),
                  "blurred_frames": sum(1 for p in prm if p & 15)}
        print("augment batch %d: %.4f ms, %.1f MB required, %.3f TB/s (%d of %d frames blurred)"
              % (N, ms, need / 1e6, need / ms / 1e9, res[N]["blurred_frames"], N))
        if not hasattr(lib, "yf_augment_warp_u8"):
            continue
        from yolo_fastest_amd.dataset import DetectDataset
        draw = DetectDataset.__new__(DetectDataset)                    # the draws alone: no files behind it
        draw.input_shape = [256, 320, 1]
        for key in ("degrees", "translate", "scale", "shear", "perspective"):
            setattr(draw, key, GEOMETRIC[key])
        random.seed(0)
        coeffs = [draw._draw_warp()[2] for _ in range(N)]
        d_warp = torch.tensor(np.stack(coeffs), dtype=torch.float64).to(dev)
        d_prm2 = torch.tensor([p | (int(rng.random() < GEOMETRIC["flipud"]) << 9) | (3 << 10) for p in prm], dtype=torch.int32, device=dev)
        scratch = torch.empty((N, 256, 320, 1), dtype=torch.uint8, device=dev)

        def launch_warp():
            _lib.check(lib.yf_augment_warp_u8(dev.index, src.data_ptr(), 512, 640, 3, None, N, N, None, None, 256, 320, 1, 15, d_prm2.data_ptr(),
                                              d_warp.data_ptr(), scratch.data_ptr(), None, x.data_ptr(), stream))
        for _ in range(5):
            launch_warp()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.reps):
            launch_warp()
        e1.record()
        torch.cuda.synchronize()
        ms2 = e0.elapsed_time(e1) / a.reps
        res[N].update(geometric_ms=round(ms2, 4), geometric_over_plain=round(ms2 / ms, 3))
        print("augment batch %d, geometric keys active (two launches): %.4f ms = %.2f x the plain launch" % (N, ms2, ms2 / ms))
    return res


def kernel_bench_mixup():
    """The plain launch, the warp call (two launches: resize + warp) and the mix call (one launch over the warp call's resized frames;
    with the resize launch in front of it as well), `--rounds` interleaved rounds of `--reps` launches each."""
    from yolo_fastest_amd.dataset import DetectDataset
    lib = _lib.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    res = {}
    for N in (16, 512):
        src = torch.randint(0, 256, (N, 512, 640, 3), dtype=torch.uint8, device=dev)
        rng = random.Random(0)
        prm = []
        for _ in range(N):
            k = (7 if rng.random() < 0.4 else 3) if rng.random() < 0.3 else 0
            prm.append(k | (int(rng.random() < 0.5) << 8))
        draw = DetectDataset.__new__(DetectDataset)                    # the draws alone: no files behind it
        draw.input_shape = [256, 320, 1]
        for key in ("degrees", "translate", "scale", "shear", "perspective"):
            setattr(draw, key, GEOMETRIC[key])
        random.seed(0)
        coeffs = np.stack([draw._draw_warp()[2] for _ in range(2 * N)]).reshape(N, 2, 8)
        ratios = [random.betavariate(32.0, 32.0) for _ in range(N)]
        prm2 = [p | (int(rng.random() < GEOMETRIC["flipud"]) << 9) | (3 << 10) for p in prm]
        d_prm = torch.tensor(prm, dtype=torch.int32, device=dev)
        d_zero = torch.zeros((N,), dtype=torch.int32, device=dev)
        d_prm2 = torch.tensor(prm2, dtype=torch.int32, device=dev)
        d_prm3 = torch.tensor([p | (3 << 12) for p in prm2], dtype=torch.int32, device=dev)
        d_warp = torch.tensor(coeffs[:, 0].copy(), dtype=torch.float64).to(dev)
        d_warp2 = torch.tensor(coeffs, dtype=torch.float64).to(dev)
        d_ratio = torch.tensor(ratios, dtype=torch.float64).to(dev)
        d_first = torch.arange(N, dtype=torch.int32, device=dev)
        d_second = torch.tensor([(n + 1) % N for n in range(N)], dtype=torch.int32, device=dev)
        scratch = torch.empty((N, 256, 320, 1), dtype=torch.uint8, device=dev)
        x = torch.empty((N, 1, 256, 320), dtype=torch.float32, device=dev)
        head = (dev.index, src.data_ptr(), 512, 640, 3, None, N, N, None, None, 256, 320, 1, 15)

        def plain():
            _lib.check(lib.yf_augment_u8(*head, d_prm.data_ptr(), None, x.data_ptr(), stream))

        def warp():
            _lib.check(lib.yf_augment_warp_u8(*head, d_prm2.data_ptr(), d_warp.data_ptr(), scratch.data_ptr(), None, x.data_ptr(), stream))

        def mix():
            _lib.check(lib.yf_augment_mix_u8(dev.index, scratch.data_ptr(), N, N, 256, 320, 1, d_first.data_ptr(), d_second.data_ptr(),
                                             d_prm3.data_ptr(), d_warp2.data_ptr(), d_ratio.data_ptr(), None, x.data_ptr(), stream))

        def resize_mix():
            _lib.check(lib.yf_augment_u8(*head, d_zero.data_ptr(), scratch.data_ptr(), None, stream))
            mix()
        calls = {"plain": plain, "warp": warp, "mix": mix, "resize+mix": resize_mix}
        for fn in calls.values():                                      # warp first: it fills the scratch the mix call reads
            for _ in range(5):
                fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = {n: [] for n in calls}
        for _ in range(a.rounds):
            for n, fn in calls.items():
                torch.cuda.synchronize()
                e0.record()
                for _ in range(a.reps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                ms[n].append(e0.elapsed_time(e1) / a.reps)
        res[N] = {n: {"median_ms": round(float(np.median(v)), 4), "rounds_ms": [round(x_, 4) for x_ in v]} for n, v in ms.items()}
        for n, v in ms.items():
            print("batch %d, %s: %.4f ms (median of %d rounds of %d launches: %s) = %.2f x the plain launch"
                  % (N, n, float(np.median(v)), len(v), a.reps, ["%.4f" % x_ for x_ in v], np.median(v) / np.median(ms["plain"])))
    return res


def kernel_bench_mosaic():
    """The plain launch, the warp call (two launches: resize + warp) and the mosaic call (one launch over the warp call's resized frames;
    with the resize launch in front of it as well), `--rounds` interleaved rounds of `--reps` launches each."""
    from yolo_fastest_amd.dataset import DetectDataset
    lib = _lib.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    res = {}
    H, W = 256, 320
    for N in (16, 512):
        src = torch.randint(0, 256, (N, 512, 640, 3), dtype=torch.uint8, device=dev)
        rng = random.Random(0)
        prm = []
        for _ in range(N):
            k = (7 if rng.random() < 0.4 else 3) if rng.random() < 0.3 else 0
            prm.append(k | (int(rng.random() < 0.5) << 8))
        draw = DetectDataset.__new__(DetectDataset)                    # the draws alone: no files behind it
        draw.input_shape = [H, W, 1]
        for key in ("degrees", "translate", "scale", "shear", "perspective"):
            setattr(draw, key, GEOMETRIC[key])
        random.seed(0)
        coeffs = np.stack([draw._draw_warp()[2] for _ in range(N)])
        canvas_coeffs = np.stack([draw._draw_warp(mosaic=True)[2] for _ in range(N)])
        centres = [[int(random.uniform(W // 2, 2 * W - W // 2)), int(random.uniform(H // 2, 2 * H - H // 2))] for _ in range(N)]
        tiles = [[n] + random.choices(range(N), k=3) for n in range(N)]
        prm2 = [p | (int(rng.random() < GEOMETRIC["flipud"]) << 9) | (3 << 10) for p in prm]
        d_prm = torch.tensor(prm, dtype=torch.int32, device=dev)
        d_zero = torch.zeros((N,), dtype=torch.int32, device=dev)
        d_prm2 = torch.tensor(prm2, dtype=torch.int32, device=dev)
        d_warp = torch.tensor(coeffs, dtype=torch.float64).to(dev)
        d_warp2 = torch.tensor(canvas_coeffs, dtype=torch.float64).to(dev)
        d_tiles = torch.tensor(tiles, dtype=torch.int32, device=dev)
        d_centre = torch.tensor(centres, dtype=torch.int32, device=dev)
        scratch = torch.empty((N, H, W, 1), dtype=torch.uint8, device=dev)
        x = torch.empty((N, 1, H, W), dtype=torch.float32, device=dev)
        head = (dev.index, src.data_ptr(), 512, 640, 3, None, N, N, None, None, H, W, 1, 15)

        def plain():
            _lib.check(lib.yf_augment_u8(*head, d_prm.data_ptr(), None, x.data_ptr(), stream))

        def warp():
            _lib.check(lib.yf_augment_warp_u8(*head, d_prm2.data_ptr(), d_warp.data_ptr(), scratch.data_ptr(), None, x.data_ptr(), stream))

        def mosaic():
            _lib.check(lib.yf_augment_mosaic_u8(dev.index, scratch.data_ptr(), N, N, H, W, 1, d_tiles.data_ptr(), d_centre.data_ptr(),
                                                d_prm2.data_ptr(), d_warp2.data_ptr(), None, x.data_ptr(), stream))

        def resize_mosaic():
            _lib.check(lib.yf_augment_u8(*head, d_zero.data_ptr(), scratch.data_ptr(), None, stream))
            mosaic()
        calls = {"plain": plain, "warp": warp, "mosaic": mosaic, "resize+mosaic": resize_mosaic}
        for fn in calls.values():                                      # warp first: it fills the scratch the mosaic call reads
            for _ in range(5):
                fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = {n: [] for n in calls}
        for _ in range(a.rounds):
            for n, fn in calls.items():
                torch.cuda.synchronize()
                e0.record()
                for _ in range(a.reps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                ms[n].append(e0.elapsed_time(e1) / a.reps)
        res[N] = {n: {"median_ms": round(float(np.median(v)), 4), "rounds_ms": [round(x_, 4) for x_ in v]} for n, v in ms.items()}
        for n, v in ms.items():
            print("batch %d, %s: %.4f ms (median of %d rounds of %d launches: %s) = %.2f x the plain launch"
                  % (N, n, float(np.median(v)), len(v), a.reps, ["%.4f" % x_ for x_ in v], np.median(v) / np.median(ms["plain"])))
    return res


def letterbox_bench(repeats=30):
    """(a), (b), (c) of the module docstring: median / min / max of `repeats` event-timed calls each, interleaved; (a) against (b) with
    the min-max spread of the two as the margin."""
    import ctypes
    from yolo_fastest_amd.training import _PinnedTable
    lib = _lib.lib()
    H, W, N = 256, 320, 256
    sizes = [(512, 640), (480, 640), (360, 640), (511, 640), (512, 1280), (640, 360), (101, 640), (253, 317)]
    g = torch.Generator().manual_seed(0)
    rng = random.Random(0)
    prm = []
    for _ in range(N):            # the reference's draws at its default probabilities (gussian_filter 0.3, fliplr 0.5)
        k = (7 if rng.random() < 0.4 else 3) if rng.random() < 0.3 else 0
        prm.append(k | (int(rng.random() < 0.5) << 8))
    res = {}
    for name, mix in (("ragged", sizes), ("uniform", [(512, 640)])):
        per = N // len(mix)
        stacks = [torch.randint(0, 256, (per,) + hw + (3,), dtype=torch.uint8, generator=g).to(dev) for hw in mix]
        pos = [[j * len(mix) + i for j in range(per)] for i in range(len(mix))]           # member j of stack i sits at batch position pos[i][j]
        ptrs, hs, ws = [0] * N, [0] * N, [0] * N
        for i, st in enumerate(stacks):
            for j, p in enumerate(pos[i]):
                ptrs[p], hs[p], ws[p] = st.data_ptr() + j * st[0].numel(), st.shape[1], st.shape[2]
        host = ((ctypes.c_void_p * N)(*ptrs), (ctypes.c_int * N)(*hs), (ctypes.c_int * N)(*ws))
        d_prm = torch.tensor(prm, dtype=torch.int32, device=dev)
        d_pos = [torch.tensor(p, device=dev) for p in pos]
        d_prm_group = [torch.tensor([prm[p] for p in ps], dtype=torch.int32, device=dev) for ps in pos]
        x = torch.empty((N, 1, H, W), dtype=torch.float32, device=dev)
        scratch = torch.empty((N, H, W, 1), dtype=torch.uint8, device=dev)
        table = _PinnedTable(_lib.YF_LB_TABLE_ENTRY_BYTES * N, dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        tabs = []
        for st in stacks:
            hw = tuple(st.shape[1:3])
            if hw in ((H, W), (2 * H, 2 * W)):
                tabs.append((None, None))
                continue
            t = torch.empty(((W + H) * 16,), dtype=torch.uint8, device=dev)
            _lib.check(lib.yf_cv_resize_tables(dev.index, hw[0], hw[1], H, W, t.data_ptr(), t.data_ptr() + W * 16, stream))
            tabs.append((t, t.data_ptr() + W * 16))

        def fused():
            _lib.check(lib.yf_augment_letterbox_u8(dev.index, N, *host, 15, H, W, d_prm.data_ptr(), 0, None, scratch.data_ptr(), None, x.data_ptr(), *table.args,
                                                   ctypes.c_void_p(stream)))

        def two_launches():
            _lib.check(lib.yf_cv_letterbox_u8(dev.index, N, *host, 15, H, W, scratch.data_ptr(), *table.args, ctypes.c_void_p(stream)))
            _lib.check(lib.yf_augment_u8(dev.index, scratch.data_ptr(), H, W, 1, None, N, N, None, None, H, W, 1, 0, d_prm.data_ptr(), None,
                                         x.data_ptr(), stream))

        def squash():
            for st, (t, yt), ps, pg in zip(stacks, tabs, d_pos, d_prm_group):
                whole = len(stacks) == 1
                dst = x if whole else torch.empty((per, 1, H, W), dtype=torch.float32, device=dev)
                _lib.check(lib.yf_augment_u8(dev.index, st.data_ptr(), st.shape[1], st.shape[2], 3, None, per, per, None if t is None else t.data_ptr(),
                                             yt, H, W, 1, 15, pg.data_ptr(), None, dst.data_ptr(), stream))
                if not whole:
                    x.index_copy_(0, ps, dst)
        cands = {"(a) yf_augment_letterbox_u8, 1 call": fused, "(b) yf_cv_letterbox_u8 + yf_augment_u8, 2 launches": two_launches,
                 "(c) squash: %d launches + %d index_copy_" % (len(stacks), 0 if len(stacks) == 1 else len(stacks)): squash}
        times = {k: [] for k in cands}
        for r in range(repeats + 3):
            for k, fn in cands.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(); e0.record(); fn(); e1.record(); torch.cuda.synchronize()   # (the sync also lets the pinned table be refilled)
                if r >= 3:
                    times[k].append(e0.elapsed_time(e1) * 1e3)
        res[name] = {}
        for k, v in times.items():
            v.sort()
            res[name][k] = {"median_us": round(float(np.median(v)), 1), "min_us": round(v[0], 1), "max_us": round(v[-1], 1)}
            print("%-8s %-58s median %8.1f us   min %8.1f   max %8.1f   (%d repeats)" % (name, k, float(np.median(v)), v[0], v[-1], len(v)))
        ka, kb = list(cands)[:2]
        ra, rb = res[name][ka], res[name][kb]
        spread = max(ra["max_us"] - ra["min_us"], rb["max_us"] - rb["min_us"])
        gain = rb["median_us"] - ra["median_us"]
        print("%-8s (b) - (a) = %.1f us of medians; min-max spread of the two: %.1f us -> (a) %s" % (
            name, gain, spread, "is faster by more than the spread" if gain > spread else "is NOT faster by more than the spread"))
        res[name]["b_minus_a_us"], res[name]["spread_us"] = round(gain, 1), round(spread, 1)
    print("(c) allocates its per-group outputs inside the timed region, as dataset.py's default path does: its figure includes the allocator")
    print("source bytes per frame vary; torch %s, HIP %s, %s" % (torch.__version__, torch.version.hip, torch.cuda.get_device_name(0)))
    return res


def profile():
    out = a.out or tempfile.mkdtemp(prefix="dataset_bench_")
    os.makedirs(out, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "aug", "--", sys.executable,
           os.path.abspath(__file__), "--kernel", "--reps", str(a.reps)]
    subprocess.check_call(cmd)
    for f in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
        with open(f) as fh:
            for row in csv.DictReader(fh):
                if "aug_kernel" in row.get("Name", ""):
                    print("rocprofv3 %s: calls %s, average %.4f ms, min %.4f ms, max %.4f ms" % (
                        row["Name"][:60], row.get("Calls"), float(row.get("AverageNs", 0)) / 1e6, float(row.get("MinNs", 0)) / 1e6,
                        float(row.get("MaxNs", 0)) / 1e6))


def voc_tree_copies(root, copies=13):
    """The 20 bundled frames with their fixture XMLs, linked `copies` times under new names: 260 items."""
    import voc_tree
    d = os.path.join(root, "train")
    os.makedirs(os.path.join(d, "img")); os.makedirs(os.path.join(d, "xml"))
    for c in range(copies):
        for s in voc_tree.bundled_stems():
            os.symlink(os.path.join(voc_tree.BUNDLED, s + ".jpg"), os.path.join(d, "img", "%s_%d.jpg" % (s, c)))
            os.symlink(os.path.join(voc_tree.VOC, "xml", s + ".xml"), os.path.join(d, "xml", "%s_%d.xml" % (s, c)))
    return d


def train_bench():
    from torch.utils.data import DataLoader
    from yolo_fastest_amd.dataset import DetectDataset
    io = yf.io_params_for(256)
    torch.manual_seed(0)
    m = yf.YoloFastest(io)
    m.initialize_weights()
    m = m.to(dev).train()
    crit = [val.YOLOLossV3(io["anchors"][i], 3, io["input_shape"], dev, model=m) for i in range(2)]
    opt = training.Adam(m.parameters(), lr=0.001)
    B = 16
    tmp = tempfile.mkdtemp()
    d = voc_tree_copies(tmp)
    aug = dict(yf.config_params["augment_params"], train_dataset_dir=d, val_dataset_dir=d)
    loaders = {}
    configs = [("cache=device", aug, dict(cache="device")), ("decode=device", aug, dict(decode="device")), ("cache=None", aug, {})]
    if hasattr(DetectDataset, "draw_ex"):
        active = dict(aug, **GEOMETRIC)
        configs += [("geometric cache=device", active, dict(cache="device")), ("geometric decode=device", active, dict(decode="device"))]
    if a.mixup:                                                          # one build: the flag unset, set with 0.0, set with 0.5
        configs = [("cache=device", aug, dict(cache="device")), ("geometric cache=device", active, dict(cache="device")),
                   ("geometric mixup=0.0 cache=device", dict(active, mixup=0.0), dict(cache="device", mixup=True)),
                   ("geometric mixup=0.5 cache=device", dict(active, mixup=0.5), dict(cache="device", mixup=True))]
    if a.mosaic:                                                         # one build: the flag unset, set with 0.0, set with 1.0
        configs = [("cache=device", aug, dict(cache="device")), ("geometric cache=device", active, dict(cache="device")),
                   ("geometric mosaic=0.0 cache=device", dict(active, mosaic=0.0), dict(cache="device", mosaic=True)),
                   ("geometric mosaic=1.0 cache=device", dict(active, mosaic=1.0), dict(cache="device", mosaic=True))]
    for name, params, kw in configs:
        ds = DetectDataset(io["input_shape"], io["origin_img_shape"], None, aug_params=params, device=dev, **kw)
        loaders[name] = DataLoader(ds, batch_size=B, num_workers=0, drop_last=True, pin_memory=True, shuffle=True, collate_fn=val.collate_fn)
    x0 = torch.rand(B, 1, 256, 320, device=dev) - 0.5
    t0 = torch.zeros(B, 64, 6, device=dev)
    t0[:, 0] = torch.tensor([0.5, 0.5, 0.1, 0.1, 1.0, 255.0])

    def batches(name):
        while True:
            if name == "no-data":
                yield x0, t0
            else:
                for imgs, targets in loaders[name]:
                    yield imgs.to(dev).float(), targets.to(dev).float()
    gens = {n: batches(n) for n in list(loaders) + ["no-data"]}
    for n, g in gens.items():                                        # warm-up: the device cache fills, engines and graphs are built
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
    print("cache=device / no-data = %.3f" % (np.median(res["cache=device"]) / np.median(res["no-data"])))
    if a.mixup:
        print("mixup 0.5 / mixup 0.0 = %.3f; mixup 0.0 / flag unset = %.3f" % (
            np.median(res["geometric mixup=0.5 cache=device"]) / np.median(res["geometric mixup=0.0 cache=device"]),
            np.median(res["geometric mixup=0.0 cache=device"]) / np.median(res["geometric cache=device"])))
    if a.mosaic:
        print("mosaic 1.0 / mosaic 0.0 = %.3f; mosaic 0.0 / flag unset = %.3f" % (
            np.median(res["geometric mosaic=1.0 cache=device"]) / np.median(res["geometric mosaic=0.0 cache=device"]),
            np.median(res["geometric mosaic=0.0 cache=device"]) / np.median(res["geometric cache=device"])))
    for n in ("cache=device", "decode=device"):
        if "geometric " + n in res and n in res and "cache=None" in res:
            print("geometric %s / %s = %.3f, / cache=None (decode=host) = %.3f" % (
                n, n, np.median(res["geometric " + n]) / np.median(res[n]), np.median(res["geometric " + n]) / np.median(res["cache=None"])))
    return {n: {"median": float(np.median(v)), "rounds": [round(float(x), 1) for x in v]} for n, v in res.items()}


out = {}
if a.letterbox:
    out["letterbox"] = letterbox_bench()
elif a.kernel and a.profile:
    profile()
elif a.kernel and a.mosaic:
    out["kernel_mosaic"] = kernel_bench_mosaic()
elif a.kernel and a.mixup:
    out["kernel_mixup"] = kernel_bench_mixup()
elif a.kernel:
    out["kernel"] = kernel_bench()
if a.train:
    out["train"] = train_bench()
if out:
    print(json.dumps(out))
