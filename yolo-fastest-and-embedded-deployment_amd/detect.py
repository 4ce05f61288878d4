"""`Detect_YOLO` -- the reference's PC inference driver (src/detect.py:87-192), batched and on the GPU.

Same constructor and `batch_detect(data_path, result_path)`; one log line per image in the reference's format
(:177,190,192).  Differences that follow from the design, not from taste:
  * frames are processed `batch_size` at a time (the reference loops one image per iteration, :146);
  * the whole of `__pre_process` behind the file decode runs on the device: cvtColor(BGR2GRAY) + cv2.resize for ANY frame size
    (yf_cv_preprocess_u8: OpenCV's 8-bit arithmetic restated -- include/yolo_fastest_hip.h; exactly 2x = the 2x2 box mean) and (u8-128)/255
    (yf_preprocess_u8); image decode uses PIL (this image has no cv2) and hands over what cv2.imread would: HWC, BGR -- or, with
    `decode="device"`, the device JPEG decoder (jpeg.py, the same bytes; baseline files, and with `progressive=True` progressive ones
    too), one decode call per batch and frame size and one
    device-to-host copy of the decoded batch for the result images;
  * model + post-process are stream-ordered launches (yf_forward, yf_decode_nms); times in the log are
    per-batch wall times divided by the batch size.
Result writer: `result_<name>` images with the reference's boxes and labels (`plot.plot_one_box`, the
reference's general.py:56-67 without cv2) and the reference's log lines; `self.last_labels` keeps the label strings per image.
`write="device"` (opt-in) draws and JPEG-encodes the result images on the device instead (plot.draw_boxes_device, jpeg.encode_batch): the
same files byte for byte, the frames never leave the GPU, and a batch is encoded while the host prepares the next one.
`letterbox=True` (opt-in) follows yolov5 where the reference squashes: every frame is letterboxed to the net's size (aspect ratio kept,
border 114; model.letterbox_u8: one launch per batch whatever the frames' sizes, where the default path pre-processes a batch of mixed
sizes frame by frame) and every box goes back to ITS frame's coordinates (post_process.scale_boxes), where the default path scales all
boxes to the configured `origin_img_shape`.
"""
import ctypes
import os
import time

import numpy as np
import torch

from . import _lib, jpeg
from .model import YoloFastest
from .plot import draw_boxes_device, plot_one_box
from .post_process import YOLO_post_process


def preprocess_u8(model, u8, input_shape):
    """Detect_YOLO.__pre_process arithmetic (detect.py:115-127) on device.
    u8: uint8 GPU tensor [N,h,w] (h,w == net input or exactly 2x) -> float32 [N,1,H,W]; a 3-channel model takes [N,h,w,3] as
    cv2.imread returns frames (BGR) -> float32 [N,3,H,W], channels reversed like `img[:, :, ::-1].transpose(2, 0, 1)` (:119)."""
    cin = model.input_channel
    want = 3 if cin == 1 else 4
    if not u8.is_cuda or u8.dtype != torch.uint8 or u8.dim() != want or (want == 4 and u8.shape[3] != cin):
        raise ValueError("expected a uint8 GPU tensor [N,h,w]" + ("" if cin == 1 else " + [%d] (HWC)" % cin))
    H, W = int(input_shape[0]), int(input_shape[1])
    N = u8.shape[0]
    e = model.engine(H, W, N, u8.device)
    x = torch.empty((N, cin, H, W), dtype=torch.float32, device=u8.device)
    u8 = u8.contiguous()
    stream = torch.cuda.current_stream(u8.device).cuda_stream
    _lib.check(e.lib.yf_preprocess_u8(e.handle, u8.data_ptr(), N, u8.shape[1], u8.shape[2], x.data_ptr(),
                                      ctypes.c_void_p(stream)))
    return x


class Detect_YOLO():
    def __init__(self, device, model_path, config_params, logger, decode="host", progressive=False, write="host", letterbox=False):
        jpeg.check_decode(decode, progressive)
        if write not in ("host", "device"):
            raise ValueError('write must be "host" or "device"')
        self.write = write
        self.letterbox = bool(letterbox)             # yolov5's letterbox + scale_boxes; `origin_img_shape` is not read in this mode
        self._label_masks = {}                       # write="device": plot.label_mask per (label, thickness), rendered once
        self._write_stream = None
        self.decode = decode
        self.progressive = bool(progressive)
        self.model = YoloFastest(config_params["io_params"]).to(device).eval()
        net_param = torch.load(model_path, map_location=device)
        self.model.load_state_dict(net_param)
        self.logger = logger
        self.device = jpeg.cuda_device(device)
        io = config_params["io_params"]
        self.class_names = io["class_names"]
        self.num_cls = io["num_cls"]
        self.nms_thres = io["nms_thre"]
        self.conf_thres = io["conf_thre"]
        self.input_shape = io["input_shape"]
        self.origin_img_shape = io["origin_img_shape"]
        self.post_process = YOLO_post_process(conf_thres=self.conf_thres, nms_thres=self.nms_thres,
                                              num_anchors=io["num_anchors"], anchors=io["anchors"],
                                              input_shape=self.input_shape, num_class=self.num_cls).bind(self.model)
        self.colors = [[106, 90, 205], [199, 97, 20], [112, 128, 105]]

    def _check_channels(self):
        if self.model.input_channel not in (1, 3):   # cv2.imread as detect.py:108-113 calls it yields 3 channels: nothing to mirror
            raise ValueError("image files decode to 3 channels; feed a %d-channel model through detect_u8" % self.model.input_channel)

    def _read_bgr(self, path):
        """-> (what cv2.imread(path) returns: uint8 [h,w,3] in BGR order, detect.py:108; the RGB original for drawing).  BGR2GRAY for a
        1-channel net (:110-111) and the resize (:115-116) happen on the device (`_pre_process`)."""
        from PIL import Image
        self._check_channels()
        ori = np.asarray(Image.open(path).convert("RGB"))
        return np.ascontiguousarray(ori[:, :, ::-1]), ori

    def _load(self, paths):
        """The files of one batch -> (their BGR frames on the device: a uint8 tensor [N, h, w, 3] if all have one size, else a list of
        [h, w, 3] tensors; with write="host" the RGB originals on the host for `_save`, else None).  `decode` says where the pixels come
        from: PIL and one upload per batch (per frame when sizes differ), or the device decoder and, for the originals, one device-to-host
        copy per frame size."""
        oris = None
        if self.decode == "device":
            self._check_channels()
            groups = jpeg.decode_files(paths, self.device, progressive=self.progressive)
            bgrs = jpeg.frames_in_order(groups)
            if self.write == "host":
                oris = [f[:, :, ::-1] for f in jpeg.frames_in_order(groups, [g.bgr.cpu().numpy() for g in groups])]
        else:
            if self.write == "host":
                host, oris = zip(*[self._read_bgr(p) for p in paths])
            else:      # each original is dropped as it is read: held for the batch they cost 0.4 ms per 640 x 512 frame (fresh host pages)
                host = [self._read_bgr(p)[0] for p in paths]
            if len({b.shape for b in host}) == 1:
                bgrs = torch.from_numpy(np.stack(host)).to(self.device)
            else:
                bgrs = [torch.from_numpy(b).to(self.device) for b in host]
        return bgrs, oris

    def _labels(self, boxes):
        """detect.py:186: the label strings of one frame's detections, as `_save` formats them."""
        return ['%s %.2f' % (self.class_names[int(b[6])], b[4] * b[5]) for b in boxes]

    def _queue_write(self, paths, frames, results, labels):
        """write="device": `_save` for one batch on a stream of its own: per frame size one copy of the frames, one draw launch
        (plot.draw_boxes_device), one encode (jpeg.encode_batch, quality 95, 4:2:0: `_save`'s arguments) and the lengths on their way to
        pinned memory.  Returns the pending item `_finish_write` turns into files; it keeps every tensor the queued work reads alive."""
        if self._write_stream is None:
            self._write_stream = torch.cuda.Stream(self.device)
        ws = self._write_stream
        ws.wait_stream(torch.cuda.current_stream(self.device))
        sizes = {}
        for i, f in enumerate(frames):
            sizes.setdefault(tuple(f.shape), []).append(i)
        parts = []
        with torch.cuda.stream(ws):
            for idx in sizes.values():
                batch = torch.stack([frames[i] for i in idx])         # a copy: the drawing is in place
                draw_boxes_device(batch, [[b[:4] for b in results[i]] for i in idx], [labels[i] for i in idx],
                                  [[self.colors[int(b[6]) % len(self.colors)] for b in results[i]] for i in idx], line_thickness=3, order="bgr",
                                  cache=self._label_masks)
                out, lengths, status = jpeg.encode_batch(batch, 95, "4:2:0", order="bgr")
                ls = torch.empty((2, len(idx)), dtype=torch.int32, pin_memory=True)
                ls[0].copy_(lengths, non_blocking=True)
                ls[1].copy_(status, non_blocking=True)
                parts.append(([paths[i] for i in idx], batch, out, ls))
            done = torch.cuda.Event()
            done.record(ws)
        return done, parts, frames

    def _finish_write(self, item):
        """Waits for a pending item of `_queue_write`, copies the used part of its encoded bytes to the host and writes the files."""
        done, parts, _ = item
        done.synchronize()
        for paths, batch, out, ls in parts:
            lengths, status = ls.tolist()
            for path, data in zip(paths, jpeg.gather_encoded(batch, out, lengths, status, 95, "4:2:0", "bgr")):
                if path is not None and os.path.isdir(os.path.dirname(path)):
                    with open(path, "wb") as f:
                        f.write(data)

    def _drain_writes(self, writes, keep=0):
        """Turns the oldest pending items of `_queue_write` into files until `keep` are left."""
        while len(writes) > keep:
            self._finish_write(writes.pop(0))

    @property
    def _origin(self):
        """The post-process' `origin_shape`: the configured original shape where it differs from the net's (__adjust_coord, :131-139)."""
        return self.origin_img_shape if list(self.input_shape[0:2]) != list(self.origin_img_shape[0:2]) else None

    def _pre_process(self, bgr):
        """detect.py:107-127 for a batch: uint8 GPU tensor [N,h,w,3] (BGR, any size) -> float32 [N,C,H,W].  The reference resizes when its
        CONFIGURED shapes differ (:115); a frame whose actual size is not the net's is resized as well (cv2.resize there would be the only
        way to feed it)."""
        u8 = self.model.cv_preprocess_u8(bgr, self.input_shape)
        return preprocess_u8(self.model, u8, self.input_shape)

    def detect_bgr_u8(self, bgr, kmax=64, gray_bits=None):
        """bgr: uint8 GPU tensor [N,h,w,3] as cv2.imread returns frames, any size.  The whole of detect.py:108-182 on the device; per-frame
        lists in the coordinates of `origin_img_shape` (after __adjust_coord, :131-139)."""
        if self.letterbox:      # `bgr` may be a list of [h,w,3] frames of any sizes; per-frame lists in each frame's own coordinates
            pred, hw = self.model.forward_letterbox_u8(bgr, self.input_shape, gray_bits=gray_bits)
            return self.post_process.detect(pred, kmax=kmax, frame_hw=hw)
        pred = self.model.forward_bgr_u8(bgr, self.input_shape, gray_bits=gray_bits)
        return self.post_process.detect(pred, kmax=kmax, origin_shape=self._origin)

    def detect_u8(self, u8, kmax=64):
        """u8: uint8 GPU tensor [N,h,w] in the ORIGINAL image geometry (any size: cv2.resize's arithmetic brings it to the net's). Returns
        per-frame lists in original coordinates (after __adjust_coord, detect.py:181-182)."""
        if self.letterbox:
            raise ValueError("detect_u8 takes one-channel frames in the original geometry; letterbox=True works on BGR frames: detect_bgr_u8")
        pred = self.model.forward_u8(u8, self.input_shape)  # pre-process in front of / fused into the first kernel's loads
        return self.post_process.detect(pred, kmax=kmax, origin_shape=self._origin)

    def batch_detect(self, data_path, result_path, batch_size=256, in_flight=2):
        """detect.py:141-192 over a directory, `batch_size` images per pass.  More than one batch: the batches go through `BatchPipeline`
        (`in_flight` of them on the GPU at a time, each on its own stream and engine -- the throughput mode bench.py measures) while the host
        decodes the next batch's files and writes the previous batch's result images; the per-image times in the log lines are then the
        batch's DEVICE times (HIP events around model and post-process, divided by the frames of the batch).  Same results, same log format
        and order as one batch at a time (`in_flight=1`)."""
        img_list = sorted(os.listdir(data_path))   # the reference iterates os.listdir order; its logs show it sorted
        num = len(img_list)
        self.last_labels = {}
        origin = None if self.letterbox else self._origin
        batches = [img_list[b0:b0 + batch_size] for b0 in range(0, num, batch_size)]
        pipelined = len(batches) > 1 and in_flight > 1
        state = {"avg": 0.0}
        writes = []                                    # write="device": pending items of _queue_write, oldest first

        def report(names, bgrs, oris, results, infer_time, post_process_time):
            total_time = infer_time + post_process_time
            state["avg"] += total_time * len(names)
            paths = [os.path.join(result_path, "result_" + n) for n in names]
            labels = [self._labels(b) for b in results]
            if self.write == "device":
                # the batch's draw + encode are queued on the writer's stream; with batches in flight the batch before it becomes files
                # now, so the GPU encodes this batch while the host decodes / packs the next one
                writes.append(self._queue_write(paths, bgrs, results, labels))
                self._drain_writes(writes, keep=int(pipelined))
            for k, (filename, boxes) in enumerate(zip(names, results)):
                if self.write == "host":
                    self._save(paths[k], oris[k], boxes)
                self.last_labels[filename] = labels[k]
                self.logger.info("image_name:%s -> %s, infer time:%.2fms, post_process time:%.2fms, total time:%.2fms"
                                 % (filename, "no targets" if len(boxes) == 0 else "detect finished", infer_time, post_process_time,
                                    total_time))

        def load(names):
            """-> (the batch's frames and originals as `_load` returns them, the net's input, with letterbox=True the frames' (h, w) on
            the device: else None)."""
            bgrs, oris = self._load([os.path.join(data_path, n) for n in names])
            if self.letterbox:      # one launch, mixed sizes or not; in flight the letterboxed u8 frames are what the batch's stream receives
                u8, hw = self.model.letterbox_u8(bgrs, self.input_shape)
                return bgrs, oris, (u8 if pipelined else preprocess_u8(self.model, u8, self.input_shape)), hw
            if not torch.is_tensor(bgrs):      # frames of different sizes: the resize brings them to one
                x = torch.cat([self._pre_process(b[None]) for b in bgrs])
            else:      # cv2.imread-shaped frames of one size; in flight, cvtColor + resize + (v - 128) / 255 run inside the batch's own stream
                x = bgrs if pipelined else self._pre_process(bgrs)
            return bgrs, oris, x, None

        if pipelined:
            from .pipeline import BatchPipeline
            saved = (self.model.lanes, self.model.branches)
            pipe = BatchPipeline(self.model, self.post_process, depth=in_flight, kmax=64, origin_shape=origin, lanes=1, branches=0)
            pending = []

            def finish(item):
                names, bgrs, oris, hw, ticket, ev = item
                raw = ticket.synchronize()
                most = int(raw["counts"].max().item()) if raw["counts"].numel() else 0
                if most > raw["boxes"].shape[1]:      # more survivors than the first attempt reserved: once more with room for all (post.detect does the same)
                    raw = self.post_process.detect_raw((raw["head_large"], raw["head_small"]), kmax=most, origin_shape=origin, frame_hw=hw)
                elif hw is not None:                  # the ticket's boxes are in net coordinates: back to each frame's own
                    self.post_process.scale_boxes(raw, hw)
                results = self.post_process.to_lists(raw)
                report(names, bgrs, oris, results, ev[0].elapsed_time(ev[1]) / len(names), ev[1].elapsed_time(ev[2]) / len(names))

            try:
                for names in batches:
                    bgrs, oris, x, hw = load(names)
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                    ev[0].record()

                    def mid(pred, ev=ev):
                        ev[1].record()
                        return pred
                    ticket = pipe.submit(x, mid=mid, then=lambda out, ev=ev: ev[2].record())
                    pending.append((names, bgrs, oris, hw, ticket, ev))
                    if len(pending) >= in_flight:
                        finish(pending.pop(0))
                while pending:
                    finish(pending.pop(0))
                self._drain_writes(writes)
            finally:
                pipe.drain()
                self.model.lanes, self.model.branches = saved
                if writes:                             # an exception on the way: nothing queued may outlive the tensors it reads
                    self._write_stream.synchronize()
                    del writes[:]
        else:
            for names in batches:
                bgrs, oris, x, hw = load(names)
                torch.cuda.synchronize(self.device)
                start_time = time.time()
                with torch.no_grad():
                    pred = self.model(x)
                torch.cuda.synchronize(self.device)
                time_mark = time.time()
                infer_time = (time_mark - start_time) * 1000 / len(names)
                results = self.post_process.detect(pred, origin_shape=origin, frame_hw=hw)
                post_process_time = (time.time() - time_mark) * 1000 / len(names)
                report(names, bgrs, oris, results, infer_time, post_process_time)
        self.logger.info("detect avg_time: %.2fms" % (state["avg"] / max(num, 1)))

    def _save(self, path, ori, boxes):
        """detect.py:184-190: one box + label per detection (plot.plot_one_box), then the image file.  Returns the label
        strings it drew ('%s %.2f' % (class name, conf * cls_score), :186)."""
        img = np.ascontiguousarray(ori).copy()
        labels = self._labels(boxes)
        for (*xyxy, _, _, cls_pred), label in zip(boxes, labels):
            # (the reference has three colours, :105, and would raise IndexError from the fourth class on: they repeat here)
            plot_one_box(xyxy, img, label=label, color=self.colors[int(cls_pred) % len(self.colors)], line_thickness=3)
        if path is not None and os.path.isdir(os.path.dirname(path)):
            from PIL import Image
            Image.fromarray(img).save(path, quality=95)   # cv2.imwrite's default JPEG quality
        return labels
