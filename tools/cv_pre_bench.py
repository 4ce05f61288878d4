"""Times yf_cv_preprocess_u8 (cvtColor + cv2.resize on the device) on a few frame geometries.  Run on the GPU box.
--letterbox: yf_cv_letterbox_u8 (model.letterbox_u8: one launch for a batch of any frame sizes) against its two yardsticks, at 320x256, gray,
256 BGR frames, HIP events around every repeat, the candidates interleaved in one process:
  uniform 480x640  (a) the letterbox launch   (b) yf_cv_preprocess_u8 squashing the same stack (table look-ups, LDS-staged rows)
  ragged, 8 sizes  (a) the letterbox launch   (a+f) followed by the (v - 128) / 255 pass   (c) Detect_YOLO's default way with mixed sizes: one
                   `_pre_process(b[None])` per frame (cv launch + float launch + allocations) and torch.cat
Prints median / min / max per candidate over the repeats, the ratios of the medians, and the launches each candidate issues."""
import os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import yolo_fastest_amd as yf
dev = torch.device("cuda:0"); io = yf.io_params_for(256)
m = yf.YoloFastest(io).to(dev).eval()
def t(x, n=20):
    for _ in range(3): m.cv_preprocess_u8(x, io["input_shape"])
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for _ in range(n): m.cv_preprocess_u8(x, io["input_shape"])
    e1.record(); torch.cuda.synchronize(); return e0.elapsed_time(e1) / n
def letterbox_bench(repeats=30):
    from yolo_fastest_amd.detect import preprocess_u8
    shape = io["input_shape"]
    sizes = [(512, 640), (480, 640), (360, 640), (511, 640), (512, 1280), (640, 360), (101, 640), (253, 317)]     # the test's sizes above 64 px a side
    g = torch.Generator().manual_seed(0)
    uniform = torch.randint(0, 256, (256, 480, 640, 3), dtype=torch.uint8, generator=g).to(dev)
    ragged = [torch.randint(0, 256, sizes[i % 8] + (3,), dtype=torch.uint8, generator=g).to(dev) for i in range(256)]
    def parent_way(frames):      # detect.py batch_detect's load() for frames of different sizes, as the default path runs it
        return torch.cat([preprocess_u8(m, m.cv_preprocess_u8(b[None], shape), shape) for b in frames])
    import ctypes
    from yolo_fastest_amd import _lib
    from yolo_fastest_amd.training import _PinnedTable
    def c_entry(frames):         # yf_cv_letterbox_u8 with its host arrays prepared once: the launch without model.letterbox_u8's Python
        n = len(frames)
        table, dst = _PinnedTable(_lib.YF_LB_TABLE_ENTRY_BYTES * n, dev), torch.empty((n, shape[0], shape[1]), dtype=torch.uint8, device=dev)
        args = (dev.index, n, (ctypes.c_void_p * n)(*[f.data_ptr() for f in frames]), (ctypes.c_int * n)(*[f.shape[0] for f in frames]),
                (ctypes.c_int * n)(*[f.shape[1] for f in frames]), m.gray_bits, shape[0], shape[1], dst.data_ptr()) + table.args
        return lambda: _lib.check(_lib.lib().yf_cv_letterbox_u8(*args, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    cands = {"uniform (a) letterbox, 1 launch": lambda: m.letterbox_u8(uniform, shape),
             "uniform (a0) the C entry alone": c_entry(list(uniform)),
             "ragged  (a0) the C entry alone": c_entry(ragged),
             "uniform (b) yf_cv_preprocess_u8, 1 launch": lambda: m.cv_preprocess_u8(uniform, shape),
             "ragged  (a) letterbox, 1 launch": lambda: m.letterbox_u8(ragged, shape),
             "ragged  (a+f) letterbox + float pass, 2 launches": lambda: preprocess_u8(m, m.letterbox_u8(ragged, shape)[0], shape),
             "ragged  (c) per frame + torch.cat, %d launches" % (2 * len(ragged) + 1): lambda: parent_way(ragged)}
    times = {k: [] for k in cands}
    for r in range(repeats + 3):
        for k, fn in cands.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(); e0.record(); fn(); e1.record(); torch.cuda.synchronize()
            if r >= 3: times[k].append(e0.elapsed_time(e1) * 1e3)
    med = {}
    for k, v in times.items():
        v = sorted(v); med[k] = v[len(v) // 2]
        print("%-52s median %8.1f us   min %8.1f   max %8.1f   (%d repeats)" % (k, med[k], v[0], v[-1], len(v)))
    ks = list(cands)
    print("uniform: (a) / (b) = %.3f, (a0) / (b) = %.3f      ragged: (c) / (a) = %.1f, (c) / (a+f) = %.1f" % (
        med[ks[0]] / med[ks[3]], med[ks[1]] / med[ks[3]], med[ks[6]] / med[ks[4]], med[ks[6]] / med[ks[5]]))
    print("source bytes: uniform %.1f MB, ragged %.1f MB; torch %s, HIP %s, %s" % (uniform.numel() / 1e6, sum(f.numel() for f in ragged) / 1e6, torch.__version__,
                                                                                  torch.version.hip, torch.cuda.get_device_name(0)))
if "--letterbox" in sys.argv:
    letterbox_bench(); sys.exit(0)
for name, shape in (("bgr 480x640", (256, 480, 640, 3)), ("bgr 512x640 (exact 1/2: area)", (256, 512, 640, 3)), ("bgr 256x320 (cvtColor only)", (256, 256, 320, 3)),
                    ("bgr 720x1280", (128, 720, 1280, 3)), ("gray 480x640", (256, 480, 640)), ("gray 128x160 (up-scaling)", (256, 128, 160)), ("bgr 481x641 (unaligned rows: byte gather)", (64, 481, 641, 3))):
    x = torch.randint(0, 256, shape, dtype=torch.uint8).to(dev); ms = t(x)
    b = x.numel() + shape[0] * 256 * 320
    print("%-44s %7.1f us  %6.0f GB/s (source + destination bytes)" % (name, ms * 1e3, b / ms / 1e6))
