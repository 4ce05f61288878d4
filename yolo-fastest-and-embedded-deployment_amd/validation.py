"""Validation-time decode + NMS on the GPU behind the reference's own names:
  `YOLOLossV3(anchors, num_classes, input_shape, device)(input)`   src/model_training/loss/yolo_loss.py:27-141 (decode branch)
  `non_max_suppression(prediction, num_classes, conf_thres, nms_thres)`   src/model_training/utils/general.py:87-143
With targets, `YOLOLossV3(...)(input, targets)` is the reference's TRAINING loss of that head (yolo_loss.py:70-97, :144-196) with an
analytic backward to the head tensor (yf_train_head_loss_ex, or yf_train_head_loss_box / _hyp with the opt-in options; SURVEY.md 8(f).4, first slice -- the layers' backward is not built).  All need an engine handle (it carries the device; the decode also needs
H and W, which come from `input_shape`).  The model is passed explicitly (`model=` / `loss.model = m`); `bind(model)` sets the
default used when none is given.  The engine is chosen by (H, W, device of the tensor) -- never "whichever exists"."""
import ctypes
import math

import torch

from . import _lib

_bound = {"model": None}


def bind(model):
    """Default model for calls that do not name one (the reference's signatures have no model argument)."""
    _bound["model"] = model


def _model(explicit):
    m = explicit if explicit is not None else _bound["model"]
    if m is None:
        raise RuntimeError("pass model=... (or call validation.bind(model) first): the kernels need an engine handle")
    return m


def _engine(t, H, W, model=None):
    if not t.is_cuda:
        raise RuntimeError("validation path (HIP) has no CPU implementation: pass GPU tensors")
    return _model(model).engine(H, W, t.shape[0], t.device)


BOX_KINDS = {"giou": 1, "diou": 2, "ciou": 3}        # YF_BOX_GIOU, YF_BOX_DIOU, YF_BOX_CIOU
# the options of yf_train_head_loss_hyp in its argument order, with their neutral values (fl_alpha is not read while fl_gamma is 0)
LOSS_HYP_DEFAULTS = (("obj_pw", 1.0), ("cls_pw", 1.0), ("label_smoothing", 0.0), ("fl_gamma", 0.0), ("fl_alpha", 0.25), ("obj_iou", 0.0),
                     ("lambda_conf", 1.0), ("lambda_cls", 1.0))


def check_loss_hyp(box_loss, obj_pw, cls_pw, label_smoothing, fl_gamma, fl_alpha, obj_iou, lambda_conf, lambda_cls):
    """ValueError for what yf_train_head_loss_hyp refuses -> the eight options as floats, in its argument order"""
    v = [float(x) for x in (obj_pw, cls_pw, label_smoothing, fl_gamma, fl_alpha, obj_iou, lambda_conf, lambda_cls)]
    for (name, _), x in zip(LOSS_HYP_DEFAULTS, v):
        if not math.isfinite(x):
            raise ValueError("%s must be finite, got %r" % (name, x))
    if v[0] <= 0 or v[1] <= 0:
        raise ValueError("obj_pw and cls_pw must be > 0, got %r and %r" % (v[0], v[1]))
    for i in (2, 4, 5):
        if not 0.0 <= v[i] <= 1.0:
            raise ValueError("%s must lie in 0 .. 1, got %r" % (LOSS_HYP_DEFAULTS[i][0], v[i]))
    if v[3] < 0 or 0 < v[3] < 1:
        raise ValueError("fl_gamma must be 0 or >= 1 (the focal derivative is unbounded at p_t = 1 in between), got %r" % v[3])
    if v[5] > 0 and box_loss is None:
        raise ValueError("obj_iou > 0 needs box_loss: the reference's four coordinate terms have no IoU value")
    if v[6] < 0 or v[7] < 0:
        raise ValueError("lambda_conf and lambda_cls must be >= 0, got %r and %r" % (v[6], v[7]))
    return tuple(v)


class YOLOLossV3(torch.nn.Module):
    def __init__(self, anchors, num_classes, input_shape, device, model=None, box_loss=None, lambda_box=5.0, obj_pw=1.0, cls_pw=1.0,
                 label_smoothing=0.0, fl_gamma=0.0, fl_alpha=0.25, obj_iou=0.0, lambda_conf=1.0, lambda_cls=1.0):
        """`box_loss` (opt-in; None = the reference's four coordinate terms, exactly as before): "giou", "diou" or "ciou" regresses the box
        of a positive cell as one IoU-family term (yf_train_head_loss_box; include/yolo_fastest_hip.h states the definition), and the
        training loss is lambda_box * box + conf + cls.  lambda_box = 5.0 is the sum of the reference's weights on x, y and on w, h;
        nobody has trained with it.  The decode (no targets) is the reference's either way.
        The eight keyword arguments behind it (opt-in; the defaults are neutral and leave the entry called above as it is) are yolov5's
        objectness / class options (yf_train_head_loss_hyp; the header states the definition): `obj_pw`, `cls_pw` the BCE positive
        weights, `label_smoothing` the eps of smooth_BCE, `fl_gamma` / `fl_alpha` the focal loss around every BCE element (gamma 0: off,
        alpha not read; 0 < gamma < 1 is refused), `obj_iou` yolov5's gr (the objectness target of a positive cell follows the clamped
        IoU value; needs `box_loss`), `lambda_conf` / `lambda_cls` plain gains on conf and cls in the total (the returned conf and cls stay
        unweighted).  yolov5's hyp files use fl_gamma 0 or 1.5 and gr 1; nothing here has been trained with any of them."""
        super().__init__()
        # the YoloFastest whose heads this decodes (None: validation.bind's default).  NOT registered as a submodule: the loss object's
        # .train() / .eval() / .to() / state_dict() must not reach into the network (the reference's YOLOLossV3 does not hold the model)
        object.__setattr__(self, "model", model)
        self.anchors = anchors
        self.num_anchors = len(anchors)
        self.num_classes = num_classes
        self.bbox_attrs = 5 + num_classes
        self.input_shape = input_shape
        self.device = device
        self.ignore_threshold = 0.5    # config_params["train_params"]["IOU_loss_thre"] (_config.py:45)
        if not (1 <= self.num_anchors <= 8) or int(num_classes) < 1:
            raise ValueError("1..8 anchors and at least one class")
        if box_loss is not None and box_loss not in BOX_KINDS:
            raise ValueError("box_loss must be None, \"giou\", \"diou\" or \"ciou\", got %r" % (box_loss,))
        if not (0.0 <= float(lambda_box) < math.inf):
            raise ValueError("lambda_box must be finite and >= 0, got %r" % (lambda_box,))
        self.box_loss = box_loss
        self.lambda_box = float(lambda_box)
        self.loss_hyp = check_loss_hyp(box_loss, obj_pw, cls_pw, label_smoothing, fl_gamma, fl_alpha, obj_iou, lambda_conf, lambda_cls)

    def forward(self, input, targets=None):
        if targets is not None:
            return self._train_loss(input, targets)
        x = input.contiguous().float()
        bs, _, fh, fw = x.shape
        if (fh * 16, fw * 16) != (int(self.input_shape[0]), int(self.input_shape[1])) and \
           (fh * 32, fw * 32) != (int(self.input_shape[0]), int(self.input_shape[1])):
            raise ValueError("head of %dx%d cells does not belong to a %s input" % (fh, fw, tuple(self.input_shape[:2])))
        m = _model(self.model)
        if x.shape[1] != self.num_anchors * self.bbox_attrs or (m.num_anchors, m.num_cls) != (self.num_anchors, self.num_classes):
            raise RuntimeError("head of %d channels / a model of %d anchors x %d classes, this loss: %d anchors x (5 + %d classes)"
                               % (x.shape[1], m.num_anchors, m.num_cls, self.num_anchors, self.num_classes))   # yolo_loss.py:58's view raises
        e = _engine(x, int(self.input_shape[0]), int(self.input_shape[1]), self.model)
        # (the reference's decode branch repeats its grid 3 times, yolo_loss.py:110-111, and only runs with 3 anchors; any count here)
        M = self.num_anchors * fh * fw
        out = torch.empty((bs, M, self.bbox_attrs), dtype=torch.float32, device=x.device)
        anc = (ctypes.c_double * (2 * self.num_anchors))(*[float(v) for a in self.anchors for v in a[:2]])
        stream = torch.cuda.current_stream(x.device).cuda_stream
        _lib.check(e.lib.yf_val_decode_head(e.handle, x.data_ptr(), bs, fh, fw, anc, M, 0, out.data_ptr(), ctypes.c_void_p(stream)))
        return out


class _TrainLossFn(torch.autograd.Function):
    """total loss of one head with its analytic gradient (yf_train_head_loss_ex, _box with `box_loss`, _hyp with
    a non-neutral option): `loss.backward()` reaches the head tensor."""

    @staticmethod
    def forward(ctx, x, targets, loss_mod):
        bs, _, fh, fw = x.shape
        H, W = int(loss_mod.input_shape[0]), int(loss_mod.input_shape[1])
        lib = _lib.lib()                                     # no inference engine needed: the loss takes (device, H, W)
        dev_index = x.device.index if x.device.index is not None else torch.cuda.current_device()
        need = ctypes.c_size_t()
        na, nc = loss_mod.num_anchors, loss_mod.num_classes
        box = loss_mod.box_loss
        hyp = loss_mod.loss_hyp
        if all(v == d for v, (name, d) in zip(hyp, LOSS_HYP_DEFAULTS) if name != "fl_alpha"):
            hyp = None                                       # every option neutral: exactly the entries below
        # the workspace size, the entry and what it takes behind the stream
        if hyp is not None:
            size_fn, loss_fn = lib.yf_train_head_loss_hyp_workspace_bytes, lib.yf_train_head_loss_hyp
            tail = (BOX_KINDS[box] if box else 0, loss_mod.lambda_box) + tuple(hyp)
        elif box is None:
            size_fn, loss_fn, tail = lib.yf_train_head_loss_workspace_bytes_ex, lib.yf_train_head_loss_ex, ()
        else:
            size_fn, loss_fn = lib.yf_train_head_loss_box_workspace_bytes, lib.yf_train_head_loss_box
            tail = (BOX_KINDS[box], loss_mod.lambda_box)
        _lib.check(size_fn(bs, fh, fw, na, nc, ctypes.byref(need)))
        work = torch.empty((need.value + 7) // 8, dtype=torch.float64, device=x.device)     # 8-byte aligned scratch
        losses = torch.empty(8, dtype=torch.float32, device=x.device)
        grad = torch.empty_like(x)
        anc = (ctypes.c_double * (2 * na))(*[float(v) for a in loss_mod.anchors for v in a[:2]])
        stream = torch.cuda.current_stream(x.device).cuda_stream
        _lib.check(loss_fn(dev_index, H, W, x.data_ptr(), bs, fh, fw, anc, na, nc, targets.data_ptr(), targets.shape[1],
                           float(loss_mod.ignore_threshold), work.data_ptr(), work.numel() * 8, losses.data_ptr(), grad.data_ptr(),
                           ctypes.c_void_p(stream), *tail))
        ctx.save_for_backward(grad)
        ctx.mark_non_differentiable(losses)
        return losses[0].clone(), losses

    @staticmethod
    def backward(ctx, g_total, _g_losses):
        (grad,) = ctx.saved_tensors
        return grad * g_total, None, None


def _train_loss(self, input, targets):
    """yolo_loss.py:70-97 with targets: (loss, x, y, w, h, conf, cls) -- loss a 0-dim tensor whose backward() fills input.grad, the rest
    Python floats like the reference's .item() values; with `box_loss`: (loss, box, 0.0, 0.0, 0.0, conf, cls).  A target whose cell lies outside the feature map or whose class lies outside
    0 .. num_classes-1 raises IndexError like the reference's indexing (a negative index wraps round there; here it raises too)."""
    if input.dim() != 4 or input.shape[1] != self.num_anchors * self.bbox_attrs:
        raise RuntimeError("input must be [batch, %d x (5 + %d), h, w]" % (self.num_anchors, self.num_classes))   # yolo_loss.py:58's view
    if not input.is_cuda:
        raise RuntimeError("training loss (HIP) has no CPU implementation: pass GPU tensors")
    x = input if (input.is_contiguous() and input.dtype == torch.float32) else input.contiguous().float()
    t = targets.to(x.device).contiguous().float()
    if t.dim() != 3 or t.shape[0] != x.shape[0] or t.shape[2] != 6:
        raise ValueError("targets must be [batch, T, 6] = (x, y, w, h, class, marker)")
    loss, parts = _TrainLossFn.apply(x, t, self)
    v = parts.tolist()
    if v[7] > 0:
        raise IndexError("%d target(s) fall outside the %dx%d feature map or name a class outside 0 .. %d"
                         % (int(v[7]), x.shape[2], x.shape[3], self.num_classes - 1))
    return loss, v[1], v[2], v[3], v[4], v[5], v[6]


YOLOLossV3._train_loss = _train_loss


def _nms_device(prediction, num_classes, conf_thres, nms_thres, kmax, model):
    """yf_val_nms_ex on the current stream -> (det float32 [bs, kmax, 7], cnt int32 [bs], kmax), all on the device, nothing read back."""
    if not prediction.is_cuda:
        raise RuntimeError("validation path (HIP) has no CPU implementation: pass GPU tensors")
    p = prediction.contiguous().float()
    bs, M, attrs = p.shape
    if int(num_classes) < 1 or attrs != 5 + int(num_classes):
        raise ValueError("prediction rows have %d values, 5 + num_classes = %d" % (attrs, 5 + int(num_classes)))
    e = _model(model).engine_on(p.device)   # yf_val_nms is size-agnostic: any engine of that model on the tensor's device
    kmax = kmax or M
    det = torch.empty((bs, kmax, 7), dtype=torch.float32, device=p.device)
    cnt = torch.empty((bs,), dtype=torch.int32, device=p.device)
    stream = torch.cuda.current_stream(p.device).cuda_stream
    _lib.check(e.lib.yf_val_nms_ex(e.handle, p.data_ptr(), bs, M, int(num_classes), float(conf_thres), float(nms_thres), kmax, det.data_ptr(),
                                   cnt.data_ptr(), ctypes.c_void_p(stream)))
    return det, cnt, kmax


def non_max_suppression(prediction, num_classes, conf_thres=0.5, nms_thres=0.4, kmax=None, model=None):
    """-> list with one [n,7] tensor (x1,y1,x2,y2,obj_conf,class_conf,class_pred) or None per image, like the reference.
    (The reference also overwrites prediction[..., :4] with the corners in place; this does not touch its input.)"""
    det, cnt, kmax = _nms_device(prediction, num_classes, conf_thres, nms_thres, kmax, model)
    counts = cnt.cpu().tolist()
    if max(counts) > kmax:
        raise OverflowError("more than kmax detections in an image")
    return [det[i, :n].clone() if n else None for i, n in enumerate(counts)]


def _nms_v5_device(prediction, conf_thres, iou_thres, agnostic, multi_label, max_det, max_nms):
    """yf_val_nms_v5 on the current stream -> (det float32 [bs, max_det, 7], cnt int32 [bs], kmax = max_det) in `_nms_device`'s layout, all
    on the device, nothing read back.  cnt never exceeds kmax."""
    if not prediction.is_cuda:
        raise RuntimeError("validation path (HIP) has no CPU implementation: pass GPU tensors")
    p = prediction.contiguous().float()
    bs, M, attrs = p.shape
    nc = attrs - 5
    if nc < 1 or bs < 1 or M < 1:
        raise ValueError("prediction must be [images >= 1, rows >= 1, 5 + classes] with at least one class, got %s" % (tuple(p.shape),))
    if not 0.0 <= float(conf_thres) <= 1.0 or not 0.0 <= float(iou_thres) <= 1.0:       # yolov5's own asserts
        raise ValueError("conf_thres and iou_thres must lie in 0 .. 1, got %r and %r" % (conf_thres, iou_thres))
    kmax, max_nms = int(max_det), int(max_nms)
    if kmax < 1 or max_nms < 1:
        raise ValueError("max_det and max_nms must be at least 1, got %r and %r" % (max_det, max_nms))
    lib = _lib.lib()
    index = p.device.index if p.device.index is not None else torch.cuda.current_device()
    need = lib.yf_val_nms_v5_work_bytes(bs, M, nc, int(bool(multi_label)))
    if not need:
        raise ValueError("%d rows x %d classes is more than 2^31 - 1 candidates" % (M, nc))
    work = torch.empty((need + 7) // 8, dtype=torch.int64, device=p.device)                # 8-byte aligned scratch
    det = torch.empty((bs, kmax, 7), dtype=torch.float32, device=p.device)
    cnt = torch.empty((bs,), dtype=torch.int32, device=p.device)
    stream = torch.cuda.current_stream(p.device).cuda_stream
    _lib.check(lib.yf_val_nms_v5(index, p.data_ptr(), bs, M, nc, float(conf_thres), float(iou_thres), int(bool(multi_label)),
                                 int(bool(agnostic)), kmax, max_nms, kmax, work.data_ptr(), work.numel() * 8, det.data_ptr(), cnt.data_ptr(),
                                 ctypes.c_void_p(stream)))
    return det, cnt, kmax


def non_max_suppression_v5(prediction, conf_thres=0.25, iou_thres=0.45, agnostic=False, multi_label=False, max_det=300, max_nms=30000,
                           model=None):
    """Not in the reference: yolov5's non_max_suppression (v6.1 / v7.0; include/yolo_fastest_hip.h: yf_val_nms_v5 states the rule) on
    decoded rows [bs, M, 5 + C] -> a list with one [n, 6] tensor (x1, y1, x2, y2, conf = obj * cls, cls) per image, confidence-descending,
    an empty [0, 6] one where nothing is kept: yolov5's return shape.  Not built: `classes`, `labels`, `merge`, the time limit.  `model`
    is there for `non_max_suppression`'s call shape only: the entry needs no engine, the device is the tensor's."""
    det, cnt, _ = _nms_v5_device(prediction, conf_thres, iou_thres, agnostic, multi_label, max_det, max_nms)
    out = torch.cat((det[..., :4], det[..., 4:5] * det[..., 5:6], det[..., 6:7]), 2)       # slots past the count hold garbage: cut below
    return [out[i, :n].clone() for i, n in enumerate(cnt.cpu().tolist())]


NMS_KINDS = ("reference", "yolov5")


def _key_fallback(t):
    """the sort key of validate.py:72 for one confidence (a 0-dim tensor): its printed form"""
    return str(t)


def _conf_keys(conf):
    """[str(c) for c in conf] for a 1-D float32 host tensor, without printing a tensor per value.  With torch's default print options a
    float32 scalar v in [0, 1] prints as 'tensor(0.)' / 'tensor(1.)' if it is integral, 'tensor(%.4e)' if v < 1e-4 (torch's sci_mode rule
    for a single value), else 'tensor(%.4f)', all from float(v).  Anything else -- other print options, another default dtype (str() then
    names float32), NaN, -0.0, values outside [0, 1] -- goes through str() itself."""
    opts = torch._tensor_str.PRINT_OPTS
    fast = opts.precision == 4 and opts.sci_mode is None and torch.get_default_dtype() == torch.float32 and conf.dtype == torch.float32
    keys = []
    for i, v in enumerate(conf.tolist()):
        if fast and 0.0 < v < 1.0:
            keys.append("tensor(%.4e)" % v if v < 1e-4 else "tensor(%.4f)" % v)
        elif fast and (v == 1.0 or (v == 0.0 and math.copysign(1.0, v) > 0)):
            keys.append("tensor(%.0f.)" % v)
        else:
            keys.append(_key_fallback(conf[i]))
    return keys


def match_iouv_image(det, targets, thr):
    """yf_val_match_iouv's rule (include/yolo_fastest_hip.h) for one image on the host, numpy float32 in the kernel's operation order:
    det [n, 7] as yf_val_nms_ex leaves it, targets [T, 6] recovered corners, thr float32 [nthr] -> hit masks int32 [n]."""
    import numpy as np
    det, targets = np.asarray(det, np.float32).reshape(-1, 7), np.asarray(targets, np.float32).reshape(-1, 6)
    n, T = len(det), len(targets)
    hit = np.zeros(n, np.int32)
    if not n or not T:
        return hit
    d, t = det[:, None, :], targets[None, :, :]
    with np.errstate(all="ignore"):
        iw = np.minimum(d[..., 2], t[..., 2]) - np.maximum(d[..., 0], t[..., 0])          # np.minimum / np.maximum hand NaN on, as torch
        ih = np.minimum(d[..., 3], t[..., 3]) - np.maximum(d[..., 1], t[..., 1])
        inter = np.where(iw < 0, np.float32(0), iw) * np.where(ih < 0, np.float32(0), ih)
        a_t = (t[..., 2] - t[..., 0]) * (t[..., 3] - t[..., 1])
        a_d = (d[..., 2] - d[..., 0]) * (d[..., 3] - d[..., 1])
        iou = inter / ((a_t + a_d) - inter + np.float32(1e-7))
        ok = (t[..., 5] > 1) & (t[..., 4] == d[..., 6]) & ~np.isnan(iou)
        has = ok.any(1)
        best = np.where(ok, iou, -np.inf).max(1)
        bt = (ok & (iou == best[:, None])).argmax(1)                                       # the lowest index among equals
        slots = np.arange(n)
        for j, th in enumerate(np.asarray(thr, np.float32)):
            cand = has & (best >= th)
            winner = np.full(T, n)
            np.minimum.at(winner, bt[cand], slots[cand])
            hit |= (cand & (winner[bt] == slots)).astype(np.int32) << j
    return hit


def collate_fn(batch):
    """What the reference's DetectDataset.collate_fn does (dataloader/detect_dataset.py:106-117): stack (h,w,c) images and
    (64,6) boxes, NHWC -> NCHW, divide the images by 255.  A batch that dataset.DetectDataset.__getitems__ built already (device
    images, host boxes) passes through."""
    import numpy as np
    from .dataset import DetectBatch
    if isinstance(batch, DetectBatch):
        return batch
    images = np.concatenate([[img] for img, _ in batch], axis=0).transpose(0, 3, 1, 2)
    bboxes = np.concatenate([[box] for _, box in batch], axis=0)
    return torch.from_numpy(images).div(255.0), torch.from_numpy(bboxes)


class Validation:
    """Mirror of the reference's `Validation` (src/model_training/validate.py:8-122): same constructor, `get_mAP(model,
    epoch)`, `clear()`, same log lines.  Model forward, decode and NMS run on the GPU (this package's kernels, one batch at a
    time); the matching and the AP arithmetic are the reference's host bookkeeping with its exact conventions:
      * targets: normalised (xc, yc, w, h, cls, marker > 1) -> input-image corners (:112-122);
      * a prediction matches the FIRST remaining same-class target with IoU (+1 pixel convention, general.py:29-52) > the
        threshold; the matched target is removed (:62-70);
      * each class's list is sorted by the PRINTED form of the confidence ('tensor(0.8714)': the reference stores
        np.array([t[4], 'TP']), a string array, and sorts that, :77) -- 4 decimals, lexicographic, stable;
      * recall is float32 (target_num is a float32 tensor), precision a Python float; equal consecutive recalls keep the
        larger precision; AP = sum over the P-R points of (recall step) x (max precision from that point on) (:87-119).
    `dataset` is anything a DataLoader accepts; items are ((h,w,c) image, (64,6) boxes) like DetectDataset's, batched with
    `collate_fn` above (images / 255) -- dataset.DetectDataset(..., val=True, augment=False) itself, batch by batch on the GPU.
    `match="device"` (not in the reference; default "host"): the matching runs on the GPU too (yf_val_match behind the NMS, one launch per
    batch, no read-back per batch); the (confidence, class, hit) records read back after the last batch rebuild the same `match_list`,
    sort keys included (`_conf_keys`), and the same `target_num`, so everything from the sort on is the code below either way.
    `get_metrics` (not in the reference either) scores the same pass as yolov5 does; it reads and changes none of `get_mAP`'s state."""

    def __init__(self, params, logger, dataset, device, model_loss, match="host"):
        from torch.utils.data import DataLoader
        if match not in ("host", "device"):
            raise ValueError("match must be 'host' or 'device', not %r" % (match,))
        self.match = match
        self._record_capacity = 1 << 20           # match="device": records the buffer of one get_mAP starts with (12 bytes each)
        self.logger = logger
        self.model_loss = model_loss
        self.device = device
        self.bs = params["train_params"]["batch_size"]
        self.input_shape = params["io_params"]["input_shape"]
        self.num_cls = params["io_params"]["num_cls"]
        self.cls_name = params["io_params"]["class_names"]
        self.IOU_threshold = params["train_params"]["IOU_val_thre"]
        self.conf_thres = params["io_params"]["conf_thre"]
        self.nms_thres = params["io_params"]["nms_thre"]
        self.dataloader = DataLoader(dataset, batch_size=self.bs, num_workers=0, drop_last=True, pin_memory=True, shuffle=True,
                                     collate_fn=collate_fn)
        self.target_num = torch.zeros((self.num_cls))
        self.match_list = [[] for _ in range(self.num_cls)]

    def clear(self):
        self.match_list = [[] for _ in range(self.num_cls)]
        self.target_num.zero_()

    def _recover_targets(self, targets):
        in_h, in_w = self.input_shape[0], self.input_shape[1]
        t = targets.clone()
        t[:, :, (0, 2)] = t[:, :, (0, 2)] * in_w
        t[:, :, (1, 3)] = t[:, :, (1, 3)] * in_h
        out = t.clone()
        out[:, :, 0] = t[:, :, 0] - t[:, :, 2] / 2
        out[:, :, 1] = t[:, :, 1] - t[:, :, 3] / 2
        out[:, :, 2] = t[:, :, 0] + t[:, :, 2] / 2
        out[:, :, 3] = t[:, :, 1] + t[:, :, 3] / 2
        return out

    @staticmethod
    def _iou(t, targets):  # general.py:29-52, float32, one prediction against all remaining targets
        ix1 = torch.max(t[0], targets[:, 0]); iy1 = torch.max(t[1], targets[:, 1])
        ix2 = torch.min(t[2], targets[:, 2]); iy2 = torch.min(t[3], targets[:, 3])
        inter = torch.clamp(ix2 - ix1 + 1, min=0) * torch.clamp(iy2 - iy1 + 1, min=0)
        a1 = (t[2] - t[0] + 1) * (t[3] - t[1] + 1)
        a2 = (targets[:, 2] - targets[:, 0] + 1) * (targets[:, 3] - targets[:, 1] + 1)
        return inter / (a1 + a2 - inter + 1e-16)

    def _match_image(self, img_pred, img_target):
        """validate.py:47-74 for one image (host tensors): img_pred [n,7] NMS output or None, img_target [64,6] recovered."""
        img_target = img_target[img_target[:, 5] > 1]
        for t in img_target:
            self.target_num[int(t[4])] += 1
        if img_pred is None:
            return
        for c in img_pred[:, 6].unique():
            target_c = img_target[img_target[:, 4] == c]
            pred_c = img_pred[img_pred[:, 6] == c]
            c = int(c)
            for t in pred_c:
                hit = False
                if target_c.size(0):
                    over = (self._iou(t, target_c) > self.IOU_threshold).nonzero()
                    if over.numel():
                        index = int(over[0])
                        target_c = torch.cat((target_c[:index], target_c[index + 1:]), dim=0)
                        hit = True
                self.match_list[c].append((str(t[4]), hit))

    def _count_targets(self, targets):
        """`target_num` of a batch of recovered targets [bs, T, 6]: what `_match_image`'s loop adds, image by image."""
        cls = targets[..., 4][targets[..., 5] > 1]
        if bool(((cls == cls.trunc()) & (cls >= 0) & (cls < self.num_cls)).all()):
            self.target_num += torch.bincount(cls.long(), minlength=self.num_cls).to(self.target_num.dtype)
        else:                                     # negative, fractional, NaN or too large: the loop's own wrap-around / exception
            for v in cls:
                self.target_num[int(v)] += 1

    def _device_records(self, model, width, nms, on_targets, launch):
        """The batches of a validation pass with the matching on the device -> the records, int32 [total, width] on the host (None if the
        loader gave no batch).  `nms(output)` is the NMS on one batch's decoded rows -> (det, cnt, kmax) on the device (`_nms_device`,
        `_nms_v5_device`).  `launch(lib, index, det, cnt, bs, kmax, t_dev, T, base, next, rec, cap, stream)` is the matching entry
        (yf_val_match, yf_val_match_iouv) on one batch; `on_targets` sees every batch's recovered host targets.  Records go to one int32
        [cap, width] buffer; the write cursor is two int64 device slots used in turn (the entry reads one and writes the other).  The
        host only keeps an upper bound of the cursor (+ bs * K_max per batch) and reads the true value -- the one synchronisation before
        the end -- when a batch could pass the capacity; the buffer is then reallocated if the batch really might not fit.  After the
        last batch two reads come back: (cursor, overflow flag) as one pair, then the filled part of the buffer."""
        lib = _lib.lib()
        dev = torch.device(self.device)
        index = dev.index if dev.index is not None else torch.cuda.current_device()
        cap = max(int(self._record_capacity), 1)
        rec = torch.empty((cap, width), dtype=torch.int32, device=dev)
        cursor = torch.zeros(2, dtype=torch.int64, device=dev)
        over = torch.zeros((), dtype=torch.int64, device=dev)    # images with more than their batch's kmax detections, summed on the stream
        bound, turn, batches = 0, 0, 0
        for imgs, targets in self.dataloader:
            targets = self._recover_targets(targets.float())                      # host, float32, as in host mode
            on_targets(targets)
            imgs = imgs.to(self.device).float()
            pred = model(imgs)
            output = torch.cat([self.model_loss[i](p) for i, p in enumerate(pred)], 1)
            det, cnt, kmax = nms(output)
            bs, T = targets.shape[0], targets.shape[1]
            if bound + bs * kmax > cap:
                bound = int(cursor[turn])                                         # the true number of records so far
                if bound + bs * kmax > cap:
                    cap = max(2 * cap, bound + bs * kmax)
                    grown = torch.empty((cap, width), dtype=torch.int32, device=dev)
                    grown[:bound] = rec[:bound]
                    rec = grown
            # a pinned staging block per batch, from torch's caching host allocator (it hands a block out again only after the copy that
            # reads it has run): ONE reused buffer would be overwritten by the next batch while its copy is still queued, since nothing
            # here waits for the stream
            t_dev = targets.contiguous().pin_memory().to(dev, non_blocking=True) if T else det   # (T = 0: never read)
            stream = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(launch(lib, index, det.data_ptr(), cnt.data_ptr(), bs, kmax, t_dev.data_ptr(), T, cursor[turn:].data_ptr(),
                              cursor[1 - turn:].data_ptr(), rec.data_ptr(), cap, ctypes.c_void_p(stream)))
            turn = 1 - turn
            bound += bs * kmax
            over += (cnt > kmax).sum()            # against THIS batch's kmax
            batches += 1
        if not batches:
            return None
        total, overflow = torch.stack((cursor[turn], over)).tolist()
        if overflow:
            raise OverflowError("more than kmax detections in an image")
        return rec[:total].cpu()

    def _match_device(self, model):
        """The batches of `get_mAP` with the matching on the device (`_device_records` with yf_val_match): records (conf bits, class, hit)."""
        thres = float(self.IOU_threshold)

        def launch(lib, index, det, cnt, bs, kmax, t_dev, T, base, nxt, rec, cap, stream):
            return lib.yf_val_match(index, det, cnt, bs, kmax, t_dev, T, thres, base, nxt, rec, cap, stream)
        def nms(output):
            return _nms_device(output, self.num_cls, self.conf_thres, self.nms_thres, None, model)
        rec = self._device_records(model, 3, nms, self._count_targets, launch)
        if rec is None:
            return
        keys = _conf_keys(rec[:, 0].contiguous().view(torch.float32))
        for key, c, hit in zip(keys, rec[:, 1].tolist(), rec[:, 2].tolist()):
            self.match_list[c].append((key, bool(hit)))

    def get_mAP(self, model, epoch):
        self.clear()
        model.eval()
        for loss in self.model_loss:
            object.__setattr__(loss, "model", model)      # (not a registered submodule, see YOLOLossV3.__init__)
        with torch.no_grad():
            if self.match == "device":
                self._match_device(model)
            else:
                for imgs, targets in self.dataloader:
                    targets = self._recover_targets(targets.float())                      # host: the bookkeeping stays on the CPU
                    imgs = imgs.to(self.device).float()
                    pred = model(imgs)
                    output = torch.cat([self.model_loss[i](p) for i, p in enumerate(pred)], 1)
                    output = non_max_suppression(output, self.num_cls, conf_thres=self.conf_thres, nms_thres=self.nms_thres, model=model)
                    output = [None if o is None else o.cpu() for o in output]
                    for img_id, img_pred in enumerate(output):
                        self._match_image(img_pred, targets[img_id])
            for c in range(self.num_cls):
                self.match_list[c].sort(key=lambda x: x[0], reverse=True)
            mAP = 0
            self.logger.info("—————— epoch: %d validation results —————" % (epoch))
            for c in range(self.num_cls):
                AP = self._calculate_AP(c)
                self.logger.info("class: %s, target_num = %d, AP = %.3f" % (self.cls_name[c], self.target_num[c], AP))
                mAP += AP
            mAP /= self.num_cls
            self.logger.info("mean AP: %.3f" % (mAP))
            self.logger.info("——————————————————————————")
        return mAP

    def get_metrics(self, model, epoch, conf_thres=0.001, nms_thres=0.6, iouv=None, nms="reference", max_det=300):
        """Not in the reference (opt-in; `get_mAP` is untouched): the pass scored as yolov5's val.py scores one -- P, R, mAP@.5 and
        mAP@.5:.95 from detections down to `conf_thres`, each matched to the targets at every IoU threshold of `iouv` (default
        torch.linspace(0.5, 0.95, 10); 1..16 finite values; "mAP@.5" is the column of iouv[0]) by process_batch's rule, ranked by
        obj_conf * class_conf (a float32 product), then metrics.ap_per_class.  Forward, decode and yf_val_nms_ex are `get_mAP`'s with
        these two thresholds, so the detections are the REFERENCE's NMS (ranked by obj_conf, +1 IoU, per class): only the scoring is
        yolov5's, and yolov5's max_det is not applied.  That is `nms="reference"`, the default.  `nms="yolov5"` takes the detections from
        yolov5's own NMS instead (yf_val_nms_v5: ranked and thresholded by obj * cls, no +1, class offsets) as val.py runs it:
        multi_label=True, agnostic only for a one-class model, max_nms=30000, `nms_thres` as its iou_thres and at most `max_det`
        detections per image -- yolov5's protocol from the logits to the table, except that val.py's rescale and clip of the boxes to
        the original image is not built (the targets here are in net-input pixels already).  `max_det` is not read with "reference".
        Matching follows `self.match`: "device" = yf_val_match_iouv behind the NMS, one
        launch per batch, records read back at the end; "host" = `match_iouv_image` per image on the NMS output.  Same records, hence
        the same numbers, either way.  Label counts come from the host targets.  Logs yolov5's table (header, an `all` row, a row per
        class; the means run over the classes that have labels, as yolov5's do) and returns {"precision", "recall", "mAP50", "mAP50_95",
        "fitness"} (floats), "ap" (float64 [num_cls, len(iouv)]) and "labels" (int64 [num_cls]).  `epoch` is there for get_mAP's
        signature; yolov5's table does not print it."""
        import numpy as np
        from . import metrics
        if iouv is None:
            iouv = torch.linspace(0.5, 0.95, 10)
        thr = [float(v) for v in iouv]
        if not 1 <= len(thr) <= 16 or not all(math.isfinite(v) for v in thr):
            raise ValueError("iouv must hold 1 to 16 finite IoU thresholds, got %r" % (thr,))
        if nms not in NMS_KINDS:
            raise ValueError("nms must be 'reference' or 'yolov5', not %r" % (nms,))
        if nms == "yolov5" and int(max_det) < 1:
            raise ValueError("max_det must be at least 1, got %r" % (max_det,))
        labels = np.zeros(self.num_cls, np.int64)
        seen = [0]

        def nms_device(output):                   # -> (det [bs, kmax, 7], cnt [bs], kmax) on the device
            if nms == "yolov5":
                return _nms_v5_device(output, conf_thres, nms_thres, self.num_cls == 1, True, max_det, 30000)
            return _nms_device(output, self.num_cls, conf_thres, nms_thres, None, model)

        def count(targets):                       # targets [bs, T, 6] recovered, host
            cls = targets[..., 4][targets[..., 5] > 1]
            if not bool(((cls == cls.trunc()) & (cls >= 0) & (cls < self.num_cls)).all()):
                raise ValueError("a target's class is not one of 0 .. %d" % (self.num_cls - 1))
            labels[:] += np.bincount(cls.long().numpy(), minlength=self.num_cls)
            seen[0] += targets.shape[0]
        model.eval()
        for loss in self.model_loss:
            object.__setattr__(loss, "model", model)      # (not a registered submodule, see YOLOLossV3.__init__)
        with torch.no_grad():
            if self.match == "device":
                c_thr = (ctypes.c_double * len(thr))(*thr)

                def launch(lib, index, det, cnt, bs, kmax, t_dev, T, base, nxt, rec, cap, stream):
                    return lib.yf_val_match_iouv(index, det, cnt, bs, kmax, t_dev, T, c_thr, len(thr), base, nxt, rec, cap, stream)
                rec = self._device_records(model, 4, nms_device, count, launch)
                rec = np.zeros((0, 4), np.int32) if rec is None else rec.numpy()
            else:
                thr32 = np.asarray(thr, np.float64).astype(np.float32)
                rows = [np.zeros((0, 4), np.int32)]
                for imgs, targets in self.dataloader:
                    targets = self._recover_targets(targets.float())
                    count(targets)
                    imgs = imgs.to(self.device).float()
                    pred = model(imgs)
                    output = torch.cat([self.model_loss[i](p) for i, p in enumerate(pred)], 1)
                    if nms == "yolov5":
                        det, cnt, _ = nms_device(output)
                        output = [det[i, :n] if n else None for i, n in enumerate(cnt.cpu().tolist())]
                    else:
                        output = non_max_suppression(output, self.num_cls, conf_thres=conf_thres, nms_thres=nms_thres, model=model)
                    for img_pred, img_target in zip(output, targets.numpy()):
                        if img_pred is None:
                            continue
                        d = img_pred.cpu().numpy()
                        rows.append(np.stack((d[:, 4].view(np.int32), d[:, 5].view(np.int32), d[:, 6].astype(np.int32),
                                              match_iouv_image(d, img_target, thr32)), 1))
                rec = np.concatenate(rows)
        self.metrics_detections = len(rec)                                                   # of this pass (tools/val_metrics_bench.py prints it)
        conf = rec[:, 0].copy().view(np.float32) * rec[:, 1].copy().view(np.float32)          # float32 product, formed here in both modes
        tp = ((rec[:, 3:4] >> np.arange(len(thr))) & 1).astype(bool)
        p, r, _, ap = metrics.ap_per_class(tp, conf, rec[:, 2], labels)
        have = labels > 0

        def mean(v):
            return float(v[have].mean()) if have.any() else 0.0
        out = {"precision": mean(p), "recall": mean(r), "mAP50": mean(ap[:, 0]), "mAP50_95": mean(ap.mean(1)), "ap": ap, "labels": labels}
        out["fitness"] = float(metrics.fitness(out["mAP50"], out["mAP50_95"]))
        row = "%20s" + "%11i" * 2 + "%11.3g" * 4
        self.logger.info(("%20s" + "%11s" * 6) % ("Class", "Images", "Labels", "P", "R", "mAP@.5", "mAP@.5:.95"))
        self.logger.info(row % ("all", seen[0], labels.sum(), out["precision"], out["recall"], out["mAP50"], out["mAP50_95"]))
        for c in range(self.num_cls):
            self.logger.info(row % (self.cls_name[c], seen[0], labels[c], p[c], r[c], ap[c, 0], ap[c].mean()))
        return out

    def _calculate_AP(self, cls):
        """validate.py:87-119 in one pass (running TP / FP counts instead of the reference's re-count per prefix)."""
        import numpy as np
        pr = []
        tp = fp = 0
        for _, is_tp in self.match_list[cls]:
            if is_tp:
                tp += 1
            else:
                fp += 1
            fn = self.target_num[cls] - tp
            if fn < 0:
                self.logger.error("error: FN less than 0!")
            precision = tp / (tp + fp)
            recall = float(tp / (tp + fn))          # float32 division, like the reference's tensor arithmetic
            if pr and recall == pr[-1][1]:
                if precision > pr[-1][0]:
                    pr[-1][0] = precision
            else:
                pr.append([precision, recall])
        ap, pre = 0, 0
        best = 0.0
        suffix_max = [0.0] * len(pr)
        for i in range(len(pr) - 1, -1, -1):
            best = max(best, pr[i][0])
            suffix_max[i] = best
        for i in range(len(pr)):
            ap += (np.float64(pr[i][1]) - pre) * suffix_max[i]
            pre = np.float64(pr[i][1])
        return ap
