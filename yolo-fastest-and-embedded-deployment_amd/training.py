"""The reference's TRAINING step on the GPU (second slice): `src/model_training/train.py:98-132`

    model.train()
    optimizer.zero_grad()
    pred = model(imgs)                                   # train-mode forward: BatchNorm on batch statistics, running stats updated
    loss = sum(model_loss[i](pred[i], targets)[0] ...)   # validation.YOLOLossV3 (yf_train_head_loss_ex / _box / _hyp)
    loss.backward()                                      # backward of every layer -> param.grad
    optimizer.step()                                     # training.Adam / training.SGD (yf_train_opt_multi_pinned) -- or any torch optimizer
    ema.update(model)                                    # opt-in, yolov5's: training.ModelEMA, inside the optimizer's launch (step(ema=...))

`YoloFastest.forward` routes here when the module is in train mode.  Forward and backward of the whole network are ONE C call each
(`yf_trainer_forward` / `yf_trainer_backward`: the graph walked in C++ over a workspace that is the pass's tape); `model.train_impl =
"ops"` selects the same computation orchestrated from Python, one C call per block (bring-up, probing).  Every operator is a HIP
kernel behind the C ABI (`yf_train_*`, csrc/yf_train_kernels.hip): Conv2d / ConvTranspose2d forward, backward-data, backward-weight; BatchNorm2d in train
mode with its backward (ReLU fused); channel slices for the torch.cat; Adam and SGD.  torch.autograd only carries the gradient across the
boundary (one Function for the whole network whose inputs are the parameters) -- no torch operator computes anything.
NCHW fp32 like the reference -- not the tuned inference engine (which folds BatchNorm into the weights and so cannot train); kernels
and measurements: DESIGN.md section 4 "The training step".  `train()` is the reference's epoch loop around the iteration,
`data_parallel()` the one-all-reduce gradient exchange for one process per GPU.  No CPU path.
"""
import ctypes

import torch

from . import _lib

_SEQ1 = ["conv0", "conv1_2", "conv1_3", "conv1_4", "res1_1", "conv1_8", "conv1_9", "conv2_1", "res2_1", "res2_2", "conv2_2", "conv2_3",
         "conv3_1", "res3_1", "res3_2", "conv3_2", "conv3_3", "conv3_4", "res3_3", "res3_4", "res3_5", "res3_6", "conv3_5", "conv3_6",
         "conv4_1", "res4_1", "res4_2", "res4_3", "res4_4", "conv4_2"]                               # yolo_fastest.py:151-190
_SEQ2 = ["conv4_3", "conv5_1", "res5_1", "res5_2", "res5_3", "res5_4", "res5_5", "conv5_2"]          # :191-200
_SEQ3 = ["conv5_3", "conv5_4", "conv5_5", "conv5_6"]                                                 # :201-204
_SEQ4 = ["conv4_1_1", "conv4_1_2", "conv4_1_3", "conv4_1_4", "conv4_1_5"]                            # :211-215


class _Ops:
    """ctypes front of the yf_train_* entry points for one device / stream."""

    def __init__(self, device):
        self.lib = _lib.lib()
        self.device = device
        self.dev = _device_index(device)
        self.stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        sc = _scratch(self.lib, device)
        self.scratch, self.scratch_bytes = sc.data_ptr(), sc.numel()
        self.bn_scratch = self.scratch

    def new(self, *shape):
        return torch.empty(shape, dtype=torch.float32, device=self.device)

    def call(self, name, *args):
        rc = getattr(self.lib, name)(self.dev, *args, self.stream)
        if rc:
            _lib.check(rc)


_SCRATCH = {}


def _scratch(lib, device):
    """The scratch of the split reductions (include/yolo_fastest_hip.h: yf_train_scratch_bytes), one per (device, stream)."""
    key = (_device_index(device), torch.cuda.current_stream(device).cuda_stream)
    if key not in _SCRATCH:
        n = ctypes.c_size_t()
        _lib.check(lib.yf_train_scratch_bytes(ctypes.byref(n)))
        _SCRATCH[key] = torch.empty(n.value, dtype=torch.uint8, device=device)
    return _SCRATCH[key]


def _device_index(device):
    return device.index if device.index is not None else torch.cuda.current_device()


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _conv_geom(conv, x):
    k, stride = conv.kernel_size[0], conv.stride[0]
    N, Cin, H, W = x.shape
    Cout = conv.out_channels
    dw = 1 if conv.groups > 1 else 0
    if dw and not (conv.groups == Cin == Cout):
        raise NotImplementedError("grouped convolution other than depthwise")
    pad = (k - 1) // 2
    return N, Cin, H, W, Cout, k, stride, dw, (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def _unit_forward(ops, mod, x, tape, name):
    """conv_norm[_relu] / deconv_norm_relu (yolo_fastest.py:16-48) in train mode: one C call (yf_train_unit_forward)."""
    conv, bn = mod[0], mod[1]
    relu = 1 if len(mod) == 3 else 0
    N, Cin, H, W = x.shape
    Cout = conv.out_channels
    if isinstance(conv, torch.nn.ConvTranspose2d):
        deconv, k, stride, dw, Ho, Wo = 1, 2, 2, 0, 2 * H, 2 * W
    else:
        deconv = 0
        _, _, _, _, _, k, stride, dw, Ho, Wo = _conv_geom(conv, x)
    zy = ops.new(2, N, Cout, Ho, Wo)
    z, y = zy[0], zy[1]
    stats = ops.new(2 * Cout)
    ops.call("yf_train_unit_forward", deconv, x.data_ptr(), conv.weight.data_ptr(), bn.weight.data_ptr(), bn.bias.data_ptr(), _ptr(bn.running_mean),
             _ptr(bn.running_var), stats.data_ptr(), z.data_ptr(), y.data_ptr(), N, Cin, H, W, Cout, k, stride, dw, relu, ops.scratch)
    if bn.num_batches_tracked is not None:
        tape.setdefault("_nbt", []).append(bn.num_batches_tracked)
    tape[name] = (x, z, y, stats, relu, (deconv, k, stride, dw))
    return y


def _unit_backward(ops, mod, tape, name, gy, grads, need_dx=True):
    conv, bn = mod[0], mod[1]
    x, z, y, stats, relu, (deconv, k, stride, dw) = tape[name]
    N, Cin, H, W = x.shape
    Cout = z.shape[1]
    gz = torch.empty_like(z)
    dgb = ops.new(2, Cout)
    dw_ = torch.empty_like(conv.weight)
    gx = torch.empty_like(x) if need_dx else None
    ops.call("yf_train_unit_backward", deconv, x.data_ptr(), z.data_ptr(), gy.data_ptr(), stats.data_ptr(), conv.weight.data_ptr(),
             bn.weight.data_ptr(), bn.bias.data_ptr(), dgb[0].data_ptr(), dgb[1].data_ptr(), gz.data_ptr(), dw_.data_ptr(), _ptr(gx), N, Cin, H, W, Cout,
             k, stride, dw, relu, ops.scratch, ops.scratch_bytes)
    grads[bn.weight], grads[bn.bias], grads[conv.weight] = dgb[0], dgb[1], dw_
    return gx


def _res_forward(ops, blk, x, tape, name):          # BasicResBlock.forward, yolo_fastest.py:60-66
    y = _unit_forward(ops, blk.conv1, x, tape, name + ".conv1")
    y = _unit_forward(ops, blk.conv2, y, tape, name + ".conv2")
    y = _unit_forward(ops, blk.conv3, y, tape, name + ".conv3")
    ops.call("yf_train_add", y.data_ptr(), x.data_ptr(), y.data_ptr(), y.numel())     # out += residual (conv3 has no ReLU: its backward
    return y                                                                            # does not read y)


def _res_backward(ops, blk, tape, name, g, grads):
    gx = _unit_backward(ops, blk.conv3, tape, name + ".conv3", g, grads)
    gx = _unit_backward(ops, blk.conv2, tape, name + ".conv2", gx, grads)
    gx = _unit_backward(ops, blk.conv1, tape, name + ".conv1", gx, grads)
    ops.call("yf_train_add", gx.data_ptr(), g.data_ptr(), gx.data_ptr(), gx.numel())
    return gx


def _run(ops, model, names, x, tape):
    for n in names:
        m = getattr(model, n)
        x = _res_forward(ops, m, x, tape, n) if n.startswith("res") else _unit_forward(ops, m, x, tape, n)
    return x


def _run_back(ops, model, names, g, tape, grads, first_needs_dx=True):
    for i in range(len(names) - 1, -1, -1):
        n = names[i]
        m = getattr(model, n)
        if n.startswith("res"):
            g = _res_backward(ops, m, tape, n, g, grads)
        else:
            g = _unit_backward(ops, m, tape, n, g, grads, need_dx=(i > 0 or first_needs_dx))
    return g


def _head_forward(ops, conv, x, tape, name):        # nn.Conv2d(C, num_out, 1) with bias, yolo_fastest.py:136 / :146
    N, Cin, H, W = x.shape
    y = ops.new(N, conv.out_channels, H, W)
    ops.call("yf_train_conv_forward", x.data_ptr(), conv.weight.data_ptr(), conv.bias.data_ptr(), y.data_ptr(), N, Cin, H, W, conv.out_channels,
             1, 1, 0)
    tape[name] = x
    return y


def _head_backward(ops, conv, tape, name, gy, grads):
    x = tape[name]
    N, Cin, H, W = x.shape
    Cout = conv.out_channels
    gy = gy.contiguous()
    dw_, db, gx = torch.empty_like(conv.weight), ops.new(Cout), torch.empty_like(x)
    ops.call("yf_train_conv_backward_weight", x.data_ptr(), gy.data_ptr(), dw_.data_ptr(), N, Cin, H, W, Cout, 1, 1, 0, ops.scratch, ops.scratch_bytes)
    ops.call("yf_train_channel_sum_split", gy.data_ptr(), db.data_ptr(), N, Cout, H * W, ops.scratch)
    ops.call("yf_train_conv_backward_data", gy.data_ptr(), conv.weight.data_ptr(), gx.data_ptr(), N, Cin, H, W, Cout, 1, 1, 0)
    grads[conv.weight], grads[conv.bias] = dw_, db
    return gx


def train_forward(model, x):
    """YoloFastest.forward (yolo_fastest.py:150-218) in train mode -> (head_large, head_small, tape)."""
    ops = _Ops(x.device)
    tape = {}
    a = _run(ops, model, _SEQ1, x, tape)                       # conv4_2
    b = _run(ops, model, _SEQ2, a, tape)                       # conv5_2
    c = _run(ops, model, _SEQ3, b, tape)
    hs = _head_forward(ops, model.head_5, c, tape, "head_5")
    d = _unit_forward(ops, model.deconv5_1, b, tape, "deconv5_1")
    N, Ca, H, W = a.shape
    Cd = d.shape[1]
    cat = ops.new(N, Ca + Cd, H, W)                            # torch.cat((conv4_2, deconv5_1), 1)
    ops.call("yf_train_channel_slice", a.data_ptr(), cat.data_ptr(), N, Ca, H * W, Ca, 0, Ca + Cd, 0)
    ops.call("yf_train_channel_slice", d.data_ptr(), cat.data_ptr(), N, Cd, H * W, Cd, 0, Ca + Cd, Ca)
    e = _run(ops, model, _SEQ4, cat, tape)
    hl = _head_forward(ops, model.head_4, e, tape, "head_4")
    tape["_cat"] = (Ca, Cd, H, W)
    if tape.get("_nbt"):
        torch._foreach_add_(tape.pop("_nbt"), 1)               # the 84 num_batches_tracked counters
    return hl, hs, tape


def train_backward(model, tape, g_hl, g_hs):
    """Backward of train_forward -> {parameter: gradient}."""
    ops = _Ops(g_hl.device)
    grads = {}
    Ca, Cd, H, W = tape["_cat"]
    N = g_hl.shape[0]
    g = _head_backward(ops, model.head_4, tape, "head_4", g_hl.float(), grads)
    g_cat = _run_back(ops, model, _SEQ4, g, tape, grads)
    g_a2, g_d = ops.new(N, Ca, H, W), ops.new(N, Cd, H, W)
    ops.call("yf_train_channel_slice", g_cat.data_ptr(), g_a2.data_ptr(), N, Ca, H * W, Ca + Cd, 0, Ca, 0)
    ops.call("yf_train_channel_slice", g_cat.data_ptr(), g_d.data_ptr(), N, Cd, H * W, Ca + Cd, Ca, Cd, 0)
    g_b2 = _unit_backward(ops, model.deconv5_1, tape, "deconv5_1", g_d, grads)
    g = _head_backward(ops, model.head_5, tape, "head_5", g_hs.float(), grads)
    g_b = _run_back(ops, model, _SEQ3, g, tape, grads)
    ops.call("yf_train_add", g_b.data_ptr(), g_b2.data_ptr(), g_b.data_ptr(), g_b.numel())
    g_a = _run_back(ops, model, _SEQ2, g_b, tape, grads)
    ops.call("yf_train_add", g_a.data_ptr(), g_a2.data_ptr(), g_a.data_ptr(), g_a.numel())
    _run_back(ops, model, _SEQ1, g_a, tape, grads, first_needs_dx=False)     # the images need no gradient
    return grads


class _Trainer:
    """yf_trainer handle for one (H, W, device): the whole forward / backward as one C call each (include/yolo_fastest_hip.h)."""

    def __init__(self, H, W, device, input_channel=1, num_out=24):
        self.lib = _lib.lib()
        self.dev = _device_index(device)
        self.handle = ctypes.c_void_p()
        _lib.check(self.lib.yf_trainer_create_ex(H, W, self.dev, int(input_channel), int(num_out), ctypes.byref(self.handle)))
        n, nb = ctypes.c_int(), ctypes.c_int()
        _lib.check(self.lib.yf_trainer_num_params(self.handle, ctypes.byref(n), ctypes.byref(nb)))
        self.n_params, self.n_bn = n.value, nb.value
        self._bytes = {}

    def layout(self, params):
        """sizes, shapes and byte offsets of the parameters in one flat buffer (the shapes of a YoloFastest never change)."""
        lay = self.__dict__.get("_layout")
        if lay is None or len(lay["sizes"]) != len(params):
            sizes = [p.numel() for p in params]
            offs, o = [], 0
            for n in sizes:
                offs.append(4 * o)
                o += n
            lay = self._layout = dict(sizes=sizes, shapes=[tuple(p.shape) for p in params], byte_offsets=offs, total=o)
        return lay

    def workspace(self, N, device):
        if N not in self._bytes:
            need = ctypes.c_size_t()
            _lib.check(self.lib.yf_trainer_workspace_bytes(self.handle, N, ctypes.byref(need)))
            self._bytes[N] = need.value
        return torch.empty(self._bytes[N], dtype=torch.uint8, device=device)     # one per forward: it is that pass's tape

    def __del__(self):
        try:
            if self.handle:
                self.lib.yf_trainer_destroy(self.handle)
        except Exception:
            pass


def _trainer(model, H, W, device):
    key = (H, W, _device_index(device))
    cache = model.__dict__.setdefault("_trainers", {})
    if key not in cache:
        cache[key] = _Trainer(H, W, device, model.input_channel, model.num_out)
    return cache[key]


def _ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _structure(model):
    """The model's parameter slots and BatchNorm modules, found once: at the reference's batch 16 an iteration is 4 ms of GPU work, and
    walking 430 modules three times per forward (parameters(), named_modules(), modules()) plus 170 `Module.__getattr__` lookups cost
    2 ms of host time -- more than the forward's kernels.  The slots are (module._parameters, name) pairs in parameters() order, so a
    replaced Parameter object is still picked up; the module SET is taken to be fixed (YoloFastest builds it in __init__)."""
    st = model.__dict__.get("_yf_struct")
    if st is None:
        slots, seen = [], set()
        for mod in model.modules():
            for name, prm in mod._parameters.items():
                if prm is not None and id(prm) not in seen:
                    seen.add(id(prm))
                    slots.append((mod._parameters, name))
        st = model.__dict__["_yf_struct"] = dict(slots=slots, bns=[m for m in model.modules() if isinstance(m, torch.nn.BatchNorm2d)],
                                                 bn_names=[n for n, m in model.named_modules() if isinstance(m, torch.nn.BatchNorm2d)])
    return st


_KEEP_TAPE = [0]     # > 0 while train_step takes the heads back one at a time: the backward only reads the tape, so it may run again


class _TrainForwardFn(torch.autograd.Function):
    """The whole network as one autograd node: inputs = the parameters, outputs = the two heads."""

    @staticmethod
    def forward(ctx, x, model, *params):
        if getattr(model, "train_impl", "trainer") == "ops":          # one C call per block, orchestrated here (kept for bring-up / probing)
            hl, hs, tape = train_forward(model, x)
            ctx.model, ctx.tape, ctx.params, ctx.tr = model, tape, params, None
            return hl, hs
        hl, hs, tr, (ws, pp) = _trainer_forward(model, x, params)
        ctx.model, ctx.tape, ctx.params, ctx.tr, ctx.params_ptr = model, (x, ws), params, tr, pp
        return hl, hs

    @staticmethod
    def backward(ctx, g_hl, g_hs):
        if ctx.tape is None:
            raise RuntimeError("backward through the training forward a second time: its saved activations were freed")
        if ctx.tr is None:
            grads = train_backward(ctx.model, ctx.tape, g_hl.contiguous(), g_hs.contiguous())
            if not _KEEP_TAPE[0]:
                ctx.tape = None
            return (None, None) + tuple(grads[p] for p in ctx.params)
        x, ws = ctx.tape
        tr, params = ctx.tr, ctx.params
        g_hl, g_hs = g_hl.contiguous().float(), g_hs.contiguous().float()
        # The C call first, the 256 gradient views after it: this runs right behind the loss's device-to-host read (the reference's
        # .item() calls), with the GPU idle until the first backward kernel is queued.  The gradients are one flat parameters()-order
        # buffer (what the trainer's single multi-tensor sum of the split weight gradients needs): pointers = base + cached offsets.
        lay = tr.layout(params)
        flat = torch.empty(lay["total"], dtype=torch.float32, device=x.device)
        base = flat.data_ptr()
        gp = (ctypes.c_void_p * len(params))(*[base + o for o in lay["byte_offsets"]])
        _lib.check(tr.lib.yf_trainer_backward(tr.handle, x.data_ptr(), g_hl.data_ptr(), g_hs.data_ptr(), x.shape[0], ctx.params_ptr,
                                              gp, ws.data_ptr(), ws.numel(),
                                              ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)))
        grads = [g.view(shp) for g, shp in zip(flat.split(lay["sizes"]), lay["shapes"])]
        if not _KEEP_TAPE[0]:
            ctx.tape = None
        sync = getattr(ctx.model, "_grad_sync", None)
        if sync is not None:                                     # data_parallel(): one all-reduce of the flat gradient buffer
            from . import dist as yfd
            yfd.all_reduce_mean_(flat, sync[0])
        return (None, None) + tuple(grads)


def _trainer_forward(model, x, params):
    N, _, H, W = x.shape
    tr = _trainer(model, H, W, x.device)
    if len(params) != tr.n_params:
        raise RuntimeError("the model has %d parameters, the trainer expects %d" % (len(params), tr.n_params))
    bns = _structure(model)["bns"]
    if len(bns) != tr.n_bn:
        raise RuntimeError("the model has %d BatchNorm layers, the trainer expects %d" % (len(bns), tr.n_bn))
    bufs = None
    bb = [b._buffers for b in bns]                           # (the dicts, not the attributes: Module.__getattr__ is 3 us a lookup)
    if all(d.get("running_mean") is not None for d in bb):
        bufs = (ctypes.c_void_p * (2 * len(bns)))(*[d[k].data_ptr() for d in bb for k in ("running_mean", "running_var")])
    hl = torch.empty((N, model.num_out, H // 16, W // 16), dtype=torch.float32, device=x.device)
    hs = torch.empty((N, model.num_out, H // 32, W // 32), dtype=torch.float32, device=x.device)
    ws = tr.workspace(N, x.device)
    pp = _ptr_array(params)
    _lib.check(tr.lib.yf_trainer_forward(tr.handle, x.data_ptr(), N, pp, bufs, hl.data_ptr(), hs.data_ptr(), ws.data_ptr(),
                                         ws.numel(), ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)))
    nbt = [d["num_batches_tracked"] for d in bb if d.get("num_batches_tracked") is not None]
    if nbt:
        torch._foreach_add_(nbt, 1)
    return hl, hs, tr, (ws, pp)


def forward(model, x):
    """model(imgs) in train mode (train.py:114)."""
    if not x.is_cuda:
        raise RuntimeError("YoloFastest training (HIP) has no CPU path: move the model and input to the GPU")
    if x.dim() != 4 or x.shape[1] != model.input_channel or x.shape[2] % 32 or x.shape[3] % 32:
        raise ValueError("expected [N,%d,H,W] with H and W multiples of 32, got %s" % (model.input_channel, tuple(x.shape)))
    st = _structure(model)
    params = [d[n] for d, n in st["slots"]]
    f32 = torch.float32
    for p in params:
        if p.dtype is not f32 or not p.is_cuda or not p.is_contiguous():
            raise RuntimeError("training runs on contiguous float32 GPU parameters")
    x = x.contiguous().float()
    for name, b in zip(st["bn_names"], st["bns"]):
        # the BatchNorm kernels (and the backward's bit-exact recomputation of the ReLU mask) are built for nn.BatchNorm2d's defaults,
        # which is what the reference uses (yolo_fastest.py:12-13): anything else would train silently wrong
        if b.eps != 1e-5 or b.momentum != 0.1 or not b.affine or not b.track_running_stats:
            raise NotImplementedError("%s: the training kernels implement BatchNorm2d(eps=1e-5, momentum=0.1, affine=True, "
                                      "track_running_stats=True) only (got eps=%r, momentum=%r, affine=%r, track_running_stats=%r)"
                                      % (name, b.eps, b.momentum, b.affine, b.track_running_stats))
    if torch.is_grad_enabled() and any(p.requires_grad for p in params):
        return _TrainForwardFn.apply(x, model, *params)
    if getattr(model, "train_impl", "trainer") == "ops":
        hl, hs, _ = train_forward(model, x)
    else:
        hl, hs, _, _ = _trainer_forward(model, x, tuple(params))
    return hl, hs


def data_parallel(model, process_group=None, broadcast=True):
    """One process per GPU (torch.distributed, backend "nccl" = RCCL): every rank trains on its shard of the batch; after this call
    `loss.backward()` averages the gradients over the ranks with ONE all-reduce of the flat gradient buffer before they reach
    `param.grad`, and the parameters and buffers are broadcast from rank 0 once.  BatchNorm uses each rank's own batch statistics
    (like torch's DistributedDataParallel without SyncBatchNorm), and -- UNLIKE DistributedDataParallel, which re-broadcasts rank 0's
    buffers before every forward -- the running_mean / running_var buffers then drift apart between the ranks: call
    `sync_buffers(model)` before validating or saving so that every rank holds rank 0's.  `train()` below does that, shards the
    data with a DistributedSampler and writes checkpoints on rank 0 only when torch.distributed is initialised.
    The reference has no distributed training; with one rank this changes nothing."""
    import torch.distributed as tdist
    if not tdist.is_initialized():
        raise RuntimeError("initialise torch.distributed first (one process per GPU)")
    from . import dist as yfd
    if broadcast:
        yfd.broadcast_model_(model, 0, process_group)
    model._grad_sync = (process_group,)
    model.train_impl = "trainer"
    return model


def sync_buffers(model, process_group=None):
    """Every rank takes rank 0's BatchNorm running statistics (what DistributedDataParallel's per-forward buffer broadcast amounts to
    at the points where the buffers are used: validation and checkpoints)."""
    import torch.distributed as tdist
    if tdist.is_initialized() and tdist.get_world_size(process_group) > 1:
        with torch.no_grad():
            for b in model.buffers():
                tdist.broadcast(b, src=0, group=process_group)
    return model


class _PinnedTable:
    """The pointer table of one multi-tensor launch: device memory, the pinned host copy the C entry fills and uploads from, the key (the
    pointers) of the last upload and that upload's event.  A class because the order matters: the C entry rewrites the pinned copy only
    when told to upload, and may do so only after the previous upload has left it."""

    def __init__(self, nbytes, device):
        self.dev = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self.host = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        self.args = (self.dev.data_ptr(), nbytes, self.host.data_ptr())      # d_table, table_bytes, h_table_pinned of the C entries
        self.key = self.event = None

    def needs_upload(self, key):
        """Whether the table on the device is not `key`'s; if so, waits until the previous upload has left the pinned copy."""
        if self.key == key:
            return False
        if self.event is not None:
            self.event.synchronize()
        return True

    def uploaded(self, key, stream):
        """The call on `stream` has uploaded `key`'s table."""
        self.key, self.event = key, torch.cuda.Event()
        self.event.record(stream)


class _MultiTensorOptimizer(torch.optim.Optimizer):
    """What training.Adam and training.SGD share: `step()` is ONE launch (yf_train_opt_multi_pinned) for every tensor of every param
    group -- the table entry of a tensor names its group, the groups' scalars (lr, weight_decay, ...) travel as kernel arguments -- when
    the tensors share a device and, for Adam, a step count; otherwise one launch per (device, step).  A torch.optim.Optimizer, so
    `param_groups[..]['lr']` edits (train.py:106-109) and `lr_scheduler.LambdaLR` (:89) work unchanged, and the state uses torch's names."""
    _kind = None

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self.__dict__.pop("_cache", None)                # the cached state tensors may have been replaced

    def _state(self, q, group):
        """-> (state tensor 1 or None, state tensor 2 or None, 1 if this is the tensor's first step of a kind the kernel must know)"""
        raise NotImplementedError

    def _scalars(self, og, group, step):
        """fill the yf_opt_group `og` from the param group"""
        raise NotImplementedError

    def _shape_key(self):
        """what, beside the participating tensors, decides which state tensors a step needs"""
        return None

    @torch.no_grad()
    def step(self, closure=None, ema=None):
        """`ema` (a ModelEMA; its model: the one it was built from or last updated with): the average is kept inside this step's launch
        -- ONE yf_train_opt_ema_multi_pinned call in which every optimised tensor carries its EMA pointer and every other floating
        state-dict entry of the model (BatchNorm running statistics, parameters without .grad) rides along as an EMA-only entry.  A step
        that needs several launches (mixed devices, Adam step counts) runs them as without `ema` and then `ema.update(model)`, a launch
        of its own.  Either way every EMA entry moves exactly once, to the bits of `step(); ema.update(model)`."""
        if closure is not None:
            raise NotImplementedError("closure")
        ema_model = ema._bound_model() if ema is not None else None
        if len(self.param_groups) > _lib.YF_OPT_MAX_GROUPS:
            raise ValueError("training.%s takes up to %d param groups (got %d)" % (type(self).__name__, _lib.YF_OPT_MAX_GROUPS, len(self.param_groups)))
        ps, gs, gof = self._taking_part()
        if not ps:
            if ema is not None:
                ema.update(ema_model)
            return
        c = self._tensor_set(ps, gof)
        gs = [g if g.is_contiguous() else g.contiguous() for g in gs]
        gp = tuple(g.data_ptr() for g in gs)
        launches = self._launches(c, ps)
        fe = self._ema_side(c, ps, ema, ema_model) if ema is not None and launches[0][2] is None else None
        for device, step, idx in launches:
            self._launch(c, gp, device, step, idx, ema, fe)
        if any(c["first"]):
            c["first"] = (0,) * len(ps)
        self._keep = gs                          # alive until the next step: the launch is asynchronous
        if ema is not None and fe is None:
            ema.update(ema_model)

    def _taking_part(self):
        """-> (parameters with a gradient, their gradients, their group indices), in group order"""
        ps, gs, gof = [], [], []
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                g = p.grad
                if g is not None:
                    ps.append(p); gs.append(g); gof.append(gi)
        return ps, gs, gof

    def _tensor_set(self, ps, gof):
        """What does not change between steps while the same Parameter objects take part: the state tensors, their pointers, the ctypes
        arrays of the one-launch case (at batch 16 the host, not the GPU, was the slower side of an iteration)."""
        c = self.__dict__.get("_cache")
        key = self._shape_key()
        n = len(ps)
        if c is None or c["gof"] != gof or c["key"] != key or any(a is not b for a, b in zip(c["ps"], ps)):
            if not all(q.is_cuda and q.dtype is torch.float32 and q.is_contiguous() for q in ps):
                raise RuntimeError("training.%s (HIP) has no CPU path: contiguous float32 GPU parameters only" % type(self).__name__)
            s1, s2, first = zip(*[self._state(q, self.param_groups[gi]) for q, gi in zip(ps, gof)])
            c = self._cache = dict(ps=list(ps), gof=gof, key=key, sts=[self.state[q] for q in ps], s1=s1, s2=s2, first=first,
                                   sizes=[q.numel() for q in ps], s1p=tuple(_ptr(t) for t in s1), s2p=tuple(_ptr(t) for t in s2), pp=None)
            c.update(s1a=(ctypes.c_void_p * n)(*c["s1p"]), s2a=(ctypes.c_void_p * n)(*c["s2p"]), na=(ctypes.c_long * n)(*c["sizes"]),
                     ga=(ctypes.c_int * n)(*gof))
        pp = tuple(q.data_ptr() for q in ps)
        if pp != c["pp"]:                                    # (a .to() / .float() of the model moves the parameters)
            c["pp"], c["pa"] = pp, (ctypes.c_void_p * n)(*pp)
        return c

    def _launches(self, c, ps):
        """-> [(device, Adam's step count or 0, the entries' indices or None for all)]; counts Adam's steps"""
        klist = None
        if self._kind == _lib.YF_OPT_ADAM:
            for st in c["sts"]:
                st["step"] = int(st["step"]) + 1             # (a loaded torch.optim.Adam state carries `step` as a tensor)
            klist = [st["step"] for st in c["sts"]]
        device = ps[0].device
        if all(q.device == device for q in ps) and (klist is None or min(klist) == max(klist)):
            return [(device, klist[0] if klist else 0, None)]     # the usual case: one launch for everything
        parts = {}                                           # mixed devices / step counts: one launch per (device, step)
        for i, q in enumerate(ps):
            parts.setdefault((q.device, klist[i] if klist else 0), []).append(i)
        return [(d, k, idx) for (d, k), idx in parts.items()]

    def _ema_side(self, c, ps, ema, ema_model):
        """The EMA's side of the one launch (_ema_fusion), kept while neither side's pointers move; None when the EMA lives elsewhere"""
        fe = c.get("ema")
        if fe is None or fe["pp"] is not c["pp"] or not ema._holds(fe):
            plan = ema._plan(ema_model)
            fe = c["ema"] = _ema_fusion(ema, plan, ps, c["pp"]) if plan["device"] == ps[0].device else None
        return fe

    def _launch(self, c, gp, device, step, idx, ema, fe):
        """One C call: the entries `idx` (None: all) on `device`, with the EMA's side `fe` behind them"""
        groups, first, ng = self.param_groups, c["first"], len(self.param_groups)
        og = (_lib.OptGroup * ng)()                          # per launch: lr is edited between steps, Adam's step differs per launch
        for gi, group in enumerate(groups):
            self._scalars(og[gi], group, step)
        if idx is None:
            m = len(gp)
            ptrs = (c["pp"], gp, c["s1p"], c["s2p"], first)
            arrs = (c["pa"], (ctypes.c_void_p * m)(*gp), c["s1a"], c["s2a"], c["na"], c["ga"], (ctypes.c_int * m)(*first))
        else:
            m = len(idx)
            ptrs = tuple(tuple(t[i] for i in idx) for t in (c["pp"], gp, c["s1p"], c["s2p"], first))
            arrs = tuple((ctypes.c_void_p * m)(*t) for t in ptrs[:4]) + ((ctypes.c_long * m)(*[c["sizes"][i] for i in idx]),
                                                                         (ctypes.c_int * m)(*[c["gof"][i] for i in idx]), (ctypes.c_int * m)(*ptrs[4]))
        # The pointer table lives on the device, with a pinned host copy, per (device, tensor count); it is re-uploaded only when
        # an entry changed (p and the state tensors never do; the gradients are views of the trainer's flat buffer, which the
        # caching allocator hands back every iteration; SGD's first-step marks fall after the first step) -- so a step is normally
        # ONE asynchronous launch and the host runs ahead.
        tables = self.__dict__.setdefault("_tables", {})
        fn, mid, tkey, nb = _lib.lib().yf_train_opt_multi_pinned, (), (device, m), _lib.YF_OPT_TABLE_ENTRY_BYTES * m
        if fe is not None:                                   # the same call with the EMA's arguments in the middle, and its own table
            ema.updates += 1
            ptrs, tkey, nb = ptrs + (fe["key"],), ("ema", device, m + fe["nx"]), _lib.YF_OPT_EMA_TABLE_ENTRY_BYTES * (m + fe["nx"])
            fn, mid = _lib.lib().yf_train_opt_ema_multi_pinned, (fe["ea"], fe["nx"], fe["xs"], fe["xe"], fe["xn"], ema.decay(ema.updates))
        table = tables.get(tkey) or tables.setdefault(tkey, _PinnedTable(nb, device))
        upload = table.needs_upload(ptrs)
        stream = torch.cuda.current_stream(device)
        _lib.check(fn(_device_index(device), self._kind, m, *arrs, ng, og, *mid, *table.args, int(upload), ctypes.c_void_p(stream.cuda_stream)))
        if upload:
            table.uploaded(ptrs, stream)
        if fe is not None:
            ema.ema._weights_dirty = True                    # the engine folds BatchNorm into a packed blob once: re-pack at the next eval forward


class Adam(_MultiTensorOptimizer):
    """`optim.Adam(model.parameters(), lr=lr0, betas=(0.9, 0.999), eps=1e-08)` (train.py:84) with the update done by one launch for all
    tensors and groups.  `weight_decay` (per group, default 0) is torch's L2 form: the gradient becomes g + weight_decay p before the
    moments, not AdamW; with 0 the update is bit for bit yf_train_adam_multi's.  State: torch's names (step, exp_avg, exp_avg_sq)."""
    _kind = _lib.YF_OPT_ADAM

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    def _state(self, q, group):
        st = self.state[q]
        if not st:
            st["step"], st["exp_avg"], st["exp_avg_sq"] = 0, torch.zeros_like(q), torch.zeros_like(q)
        return st["exp_avg"], st["exp_avg_sq"], 0

    def _scalars(self, og, group, step):
        og.lr, og.weight_decay, og.eps, og.step = float(group["lr"]), float(group.get("weight_decay", 0)), float(group["eps"]), int(step)
        og.beta1, og.beta2 = float(group["betas"][0]), float(group["betas"][1])
        if group.get("maximize") or group.get("amsgrad"):
            raise ValueError("training.Adam: maximize and amsgrad are not implemented")


class SGD(_MultiTensorOptimizer):
    """`torch.optim.SGD(params, lr, momentum, weight_decay=.., nesterov=..)` with the update done by one launch for all tensors and
    groups, bit for bit torch's arithmetic (csrc/yf_train_opt_kernels.h: tsgd_group_kernel).  State: torch's `momentum_buffer`, created at
    a tensor's first step (which stores d, without reading the buffer); no state without momentum.  No dampening, no maximize."""
    _kind = _lib.YF_OPT_SGD

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False):
        if dampening != 0:
            raise ValueError("training.SGD: dampening is not implemented")
        if momentum < 0 or lr < 0 or weight_decay < 0:
            raise ValueError("training.SGD: lr, momentum and weight_decay must not be negative")
        if nesterov and momentum <= 0:
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")         # torch's words
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov))

    def _shape_key(self):
        return tuple(g["momentum"] != 0 for g in self.param_groups)

    def _state(self, q, group):
        if group["momentum"] == 0:
            return None, None, 0
        st = self.state[q]
        buf = st.get("momentum_buffer")
        if buf is None:                                      # the first step writes it
            st["momentum_buffer"] = buf = torch.empty_like(q)
            return buf, None, 1
        return buf, None, 0

    def _scalars(self, og, group, step):
        og.lr, og.weight_decay, og.momentum = float(group["lr"]), float(group.get("weight_decay", 0)), float(group["momentum"])
        og.dampening, og.nesterov, og.maximize = float(group.get("dampening", 0)), int(bool(group.get("nesterov"))), int(bool(group.get("maximize")))
        if og.dampening != 0 or og.maximize or (og.nesterov and og.momentum <= 0):
            raise ValueError("training.SGD: dampening, maximize and nesterov without momentum are not implemented")


def _state_slots(module):
    """[(state-dict key, the owning module's _parameters / _buffers dict, name)] in state_dict() order.  The dicts, not the tensors, so a
    replaced tensor (.to(), load_state_dict of a buffer) is still picked up; the module SET is taken to be fixed, as in _structure()."""
    out = []
    for prefix, mod in module.named_modules():
        pre = prefix + "." if prefix else ""
        out += [(pre + k, mod._parameters, k) for k, v in mod._parameters.items() if v is not None]
        out += [(pre + k, mod._buffers, k) for k, v in mod._buffers.items() if v is not None and k not in mod._non_persistent_buffers_set]
    return out


def _ema_fusion(ema, plan, ps, pp):
    """The EMA's part of one fused optimizer launch: the EMA pointer of every optimised tensor `ps`, and the model's remaining floating
    entries as EMA-only (source, EMA, size) triples -- ctypes arrays, built once per (plan, tensor set) and kept while ModelEMA._holds."""
    where = {id(t): i for i, t in enumerate(plan["src"])}
    try:
        at = [where[id(q)] for q in ps]
    except KeyError:
        raise ValueError("step(ema=...): an optimised tensor is no floating state-dict entry of the EMA's model") from None
    taken = set(at)
    rest = [i for i in range(len(plan["src"])) if i not in taken]
    sp, ep, sizes, slots = plan["sp"], plan["ep"], plan["sizes"], plan["slots"]
    nx = len(rest)
    key = (tuple(ep[i] for i in at), tuple(sp[i] for i in rest), tuple(ep[i] for i in rest))
    return dict(of=ema, plan=plan, pp=pp, key=key, nx=nx, rest=[slots[i][1:] for i in rest], ea=(ctypes.c_void_p * len(at))(*key[0]),
                xs=(ctypes.c_void_p * max(nx, 1))(*key[1]), xe=(ctypes.c_void_p * max(nx, 1))(*key[2]),
                xn=(ctypes.c_long * max(nx, 1))(*[sizes[i] for i in rest]))


class ModelEMA:
    """yolov5's `ModelEMA(model, decay=0.9999, tau=2000, updates=0)`: an exponential moving average of every floating-point
    state-dict entry (this network: 256 parameters and 168 BatchNorm running statistics of 508 keys), updated after each optimizer step,

        d = decay * (1 - exp(-updates / tau));   v *= d;   v += (1 - d) * model_value          (float32, three rounded operations)

    Validation and the deployed checkpoint use the average.  `.ema` is a YoloFastest in eval mode holding it (parameters without
    gradient), built from the model's io_params and state_dict() (of any other module: a deepcopy); `.updates` counts the updates, `.decay(x)` is the ramp.  Integer
    entries (num_batches_tracked) keep the value they had at construction, as in yolov5.  `update(model)` is ONE launch over all
    floating entries (yf_train_ema_multi_pinned) where yolov5's loop takes three torch launches per entry; `optimizer.step(ema=...)` of
    training.SGD / training.Adam keeps it inside the optimizer's own launch.  No CPU path for update()."""

    _KNOBS = ("chunk", "fusion", "lanes", "branches", "split_sums", "post_split", "storage_dtype", "precision")

    def __init__(self, model, decay=0.9999, tau=2000, updates=0):
        from .model import YoloFastest
        if not (0.0 <= float(decay) <= 1.0) or not float(tau) > 0 or int(updates) < 0:
            raise ValueError("ModelEMA: decay in [0, 1], tau > 0 and updates >= 0 (got %r, %r, %r)" % (decay, tau, updates))
        if isinstance(model, YoloFastest):                   # a new network from the io_params: the model owns engine handles, no deepcopy
            # its layers draw initial values (overwritten below); the caller's random stream stays where a run without EMA has it, so
            # train(ema=True) shuffles and augments exactly as train(ema=False) does
            with torch.random.fork_rng(devices=[]):
                net = YoloFastest(dict(num_cls=model.num_cls, input_channel=model.input_channel, num_anchors=model.num_anchors,
                                       gray_bits=model.gray_bits))
            for k in self._KNOBS:
                setattr(net, k, getattr(model, k))
            first = next(model.parameters())
            net = net.to(device=first.device, dtype=first.dtype)
        else:                                                # any other module, as yolov5's class does it
            import copy
            net = copy.deepcopy(model)
        self._slots = [(k, d, n) for k, d, n in _state_slots(net) if d[n].is_floating_point()]
        self._model = self._cache = None
        self._tables = {}
        self._bind(model)
        net.load_state_dict(model.state_dict())
        for p in net.parameters():
            p.requires_grad_(False)
        self.ema = net.eval()
        self.updates, self._decay, self.tau = int(updates), float(decay), float(tau)

    def decay(self, x):
        """the decay of update number x: it ramps from 0 to `decay`, so the early averages follow the model"""
        import math
        return self._decay * (1 - math.exp(-x / self.tau))

    # -- which model -----------------------------------------------------------------------------
    def _bind(self, model):
        """`model` becomes the one update() and step(ema=...) read: its floating state-dict entries must be the EMA's, key for key and
        shape for shape (checked once per model)."""
        import weakref
        slots = model.__dict__.get("_yf_ema_slots")
        if slots is None:
            slots = [(k, d, n) for k, d, n in _state_slots(model) if d[n].is_floating_point()]
        mine = self._slots
        theirs = {k: tuple(d[n].shape) for k, d, n in slots}
        if [k for k, _, _ in slots] != [k for k, _, _ in mine]:
            odd = sorted(set(theirs) ^ {k for k, _, _ in mine})
            raise ValueError("ModelEMA: the model's floating state-dict keys are not the EMA's (%d against %d; e.g. %s)"
                             % (len(slots), len(mine), ", ".join(odd[:3]) or "another order"))
        for k, d, n in mine:
            if tuple(d[n].shape) != theirs[k]:
                raise ValueError("ModelEMA: %s is %s in the model and %s in the EMA" % (k, theirs[k], tuple(d[n].shape)))
        model.__dict__["_yf_ema_slots"] = slots
        self._model, self._cache = weakref.ref(model), None

    def _bound_model(self):
        m = self._model() if self._model is not None else None
        if m is None:
            raise RuntimeError("ModelEMA: the model it was built from is gone; call update(model) once, or train_step(..., ema=ema)")
        return m

    def _plan(self, model):
        """The pointers, sizes and ctypes arrays of one update, cached the way _MultiTensorOptimizer caches its own: rebuilt (a new dict)
        only when a tensor of either side moved."""
        if self._model is None or self._model() is not model:
            self._bind(model)
        slots = model.__dict__["_yf_ema_slots"]
        src = [d[n] for _, d, n in slots]
        sp = tuple(map(torch.Tensor.data_ptr, src))
        c = self._cache
        if c is None or c["sp"] != sp or self._moved(c):
            dst = [d[n] for _, d, n in self._slots]
            ep = tuple(map(torch.Tensor.data_ptr, dst))
            f32, device = torch.float32, dst[0].device
            for t in src + dst:
                if not t.is_cuda or t.dtype is not f32 or not t.is_contiguous() or t.device != device:
                    raise RuntimeError("ModelEMA.update (HIP) has no CPU path: contiguous float32 tensors of the model and the EMA on one GPU")
            n = len(src)
            sizes = [t.numel() for t in dst]
            c = self._cache = dict(sp=sp, ep=ep, src=src, dst=dst, slots=slots, sizes=sizes, device=device, n=n, sa=(ctypes.c_void_p * n)(*sp),
                                   ea=(ctypes.c_void_p * n)(*ep), na=(ctypes.c_long * n)(*sizes))
        return c

    def _moved(self, c):
        """Whether `.ema`'s tensors have left the addresses of plan `c`.  `.ema` is this object's own network and its tensors move only all
        at once (.to(), .half(); load_state_dict copies in place), so the first and the last entry stand for all 424: at batch 16 the
        host is the slower side of an iteration, and reading every pointer of both networks in every step showed in its time."""
        (_, d0, n0), (_, d1, n1) = self._slots[0], self._slots[-1]
        return d0[n0].data_ptr() != c["ep"][0] or d1[n1].data_ptr() != c["ep"][-1]

    def _holds(self, fe):
        """Whether the fused-launch arrays `fe` (_ema_fusion) still describe this EMA and its model: the plan is the current one, `.ema` has
        not moved, and the model's EMA-only tensors -- the optimizer has compared the pointers of its own -- are where they were."""
        return (fe["of"] is self and fe["plan"] is self._cache and not self._moved(fe["plan"])
                and tuple(map(torch.Tensor.data_ptr, [d[n] for d, n in fe["rest"]])) == fe["key"][1])

    # -- the update ------------------------------------------------------------------------------
    @torch.no_grad()
    def update(self, model):
        """yolov5's `update(model)`: `updates` += 1, then every floating entry in one launch."""
        c = self._plan(model)
        device, n = c["device"], c["n"]
        table = self._tables.get((device, n)) or self._tables.setdefault((device, n), _PinnedTable(_lib.YF_EMA_TABLE_ENTRY_BYTES * n, device))
        key = (c["sp"], c["ep"])
        upload = table.needs_upload(key)
        self.updates += 1
        stream = torch.cuda.current_stream(device)
        _lib.check(_lib.lib().yf_train_ema_multi_pinned(_device_index(device), n, c["sa"], c["ea"], c["na"], self.decay(self.updates), *table.args,
                                                        int(upload), ctypes.c_void_p(stream.cuda_stream)))
        if upload:
            table.uploaded(key, stream)
        # the easy bug: the engine folds BatchNorm into a packed blob once, and the kernel has just changed the tensors behind its back
        self.ema._weights_dirty = True

    # -- resuming --------------------------------------------------------------------------------
    def state_dict(self):
        """the EMA network's state-dict (508 keys here) plus `updates`"""
        sd = self.ema.state_dict()
        sd["updates"] = self.updates
        return sd

    def load_state_dict(self, state_dict):
        sd = dict(state_dict)
        if "updates" not in sd:
            raise ValueError("ModelEMA.load_state_dict: no 'updates' entry")
        updates = int(sd.pop("updates"))
        own = self.ema.state_dict()
        if set(sd) != set(own):
            odd = sorted(set(sd) ^ set(own))
            raise ValueError("ModelEMA.load_state_dict: %d keys against the EMA's %d (e.g. %s)" % (len(sd), len(own), ", ".join(odd[:3])))
        for k, v in own.items():
            if tuple(sd[k].shape) != tuple(v.shape):
                raise ValueError("ModelEMA.load_state_dict: %s is %s, the EMA's is %s" % (k, tuple(sd[k].shape), tuple(v.shape)))
        self.ema.load_state_dict(sd)                         # (in place, and it drops the packed weights)
        self.updates = updates


def param_groups(model, weight_decay):
    """yolov5's three optimizer groups (its train.py), by module type over named_modules(), in yolov5's order: BatchNorm2d weights (no
    decay), every other module's .weight (Conv2d, ConvTranspose2d; `weight_decay`), every .bias (BatchNorm2d's included; no decay)."""
    bn, w, b = [], [], []
    for _, mod in model.named_modules():
        if isinstance(getattr(mod, "bias", None), torch.nn.Parameter):
            b.append(mod.bias)
        if isinstance(mod, torch.nn.BatchNorm2d):
            if isinstance(mod.weight, torch.nn.Parameter):
                bn.append(mod.weight)
        elif isinstance(getattr(mod, "weight", None), torch.nn.Parameter):
            w.append(mod.weight)
    ids = [id(p) for p in bn + w + b]
    if len(set(ids)) != len(ids) or set(ids) != {id(p) for p in model.parameters()}:
        raise ValueError("param_groups: a parameter that is no module's .weight or .bias, or one shared by two modules")
    return [{"params": bn}, {"params": w, "weight_decay": weight_decay}, {"params": b}]


def train_step(model, model_loss, optimizer, imgs, targets, branch_weight=None, ema=None):
    """One iteration of train.py:111-132: returns the summed losses [total, x, y, w, h, conf, cls] (total a 0-dim tensor).
    `branch_weight` (a sequence, one factor per head; the reference sums the heads unweighted, :129-130): head i's seven values are
    multiplied by branch_weight[i] before the sum, so the backward reaches head i scaled by it.  With factors other than 1 the heads
    are taken back one at a time over the same tape and `p.grad` accumulates: every gradient is sum_i round(branch_weight[i] * g_i), g_i
    head i's own gradient, added once -- the fp32 backward of a sum of head gradients is not the sum of their backwards (it rounds at
    every accumulation), and only this form is linear in the heads to the last bit.  It costs one backward per head.  None and all-ones
    are the reference's single backward, bit for bit.
    `ema` (a ModelEMA of `model`): updated once behind the optimizer step, yolov5's `optimizer.step(); ema.update(model)` -- inside the
    optimizer's launch with training.SGD / training.Adam (`optimizer.step(ema=ema)`), as a launch of its own with any other optimizer."""
    optimizer.zero_grad()
    pred = model(imgs)
    if branch_weight is not None and len(branch_weight) != len(pred):
        raise ValueError("branch_weight has %d entries, the model %d heads" % (len(branch_weight), len(pred)))
    weights = None if branch_weight is None else [float(v) for v in branch_weight]
    losses = [[] for _ in range(7)]
    for i, item_pred in enumerate(pred):
        for j, v in enumerate(model_loss[i](item_pred, targets)):
            losses[j].append(v if weights is None else v * weights[i])
    per_head = weights is not None and any(v != 1.0 for v in weights)
    heads = losses[0] if per_head else None                  # (held only when needed: live tensors shift the allocator's pattern, and a
    losses = [sum(v) for v in losses]                        #  pass is replayed as a graph only when its pointers repeat)
    if not per_head:
        losses[0].backward()
    else:
        _KEEP_TAPE[0] += 1
        try:
            for h in heads[:-1]:
                h.backward(retain_graph=True)
        finally:
            _KEEP_TAPE[0] -= 1
        heads[-1].backward()                                 # the last one frees the tape
    if ema is None:
        optimizer.step()
    elif isinstance(optimizer, _MultiTensorOptimizer):
        if ema._model is None or ema._model() is not model:
            ema._bind(model)
        optimizer.step(ema=ema)
    else:
        optimizer.step()
        ema.update(model)
    return losses


def cosine_factor(epoch, total_epochs):
    """train.py:87-88 `lf`: the per-epoch learning-rate factor, 1.0 -> 0.2 over the run."""
    import math
    return ((1 + math.cos(epoch * math.pi / total_epochs)) / 2) * 0.8 + 0.2


# train(loss_hyp=...): yolov5's key -> validation.YOLOLossV3's keyword
LOSS_HYP_KEYS = {"obj": "lambda_conf", "cls": "lambda_cls", "obj_pw": "obj_pw", "cls_pw": "cls_pw", "fl_gamma": "fl_gamma",
                 "label_smoothing": "label_smoothing", "gr": "obj_iou", "fl_alpha": "fl_alpha"}


def train(params, device, tbwriter=None, train_dataset=None, val_dataset=None, logger=None, val_match="host", optimizer=None,
          branch_weight=False, ema=False, box_loss=None, lambda_box=5.0, val_metrics=False, val_nms="reference", loss_hyp=None,
          autoanchor=False):
    """The reference's `train(params, device, tbwriter)` (train.py:44-160) with the iteration on the GPU kernels of this package.
    Same control flow and arithmetic: one YOLOLossV3 per stride (:50-53), the model from `pretrained_pth` or initialize_weights()
    (:58-65), DataLoader(batch_size, drop_last, shuffle) (:71-73), Adam(lr0, betas (0.9, 0.999), eps 1e-8) (:84), the cosine
    LambdaLR stepped per epoch (:87-91), the linear warm-up of the first max(3 epochs, 1000 iterations) written into param_groups per
    iteration (:103-109), the log line every 10 iterations (:134-150, same format), get_mAP after epoch 4 (:153-154) and one
    `YOLO-Fastest_epoch_N.pth` state-dict per epoch (:155).  Differences: the datasets are passed in (the reference builds them from
    config paths, train.py:68-76; here: `dataset.DetectDataset(io["input_shape"], io["origin_img_shape"], logger,
    aug_params=params["augment_params"])` and the same with `augment=False, val=True`); items are DetectDataset's ((h, w, c) uint8-range
    image, (64, 6) boxes), batched by validation.collate_fn (= DetectDataset.collate_fn), or DetectDataset's whole-batch
    `__getitems__` (device images), which the collate passes through.  tbwriter may be None.  `val_match` is Validation's `match`
    ("host", the default, or "device": the TP / FP matching of get_mAP on the GPU, same result).
    Opt-in, the three train_params keys the reference carries but does not read, with yolov5's meaning (the keys come from its hyp
    files): `optimizer="adam"` = Adam(param_groups(model, weight_decay), lr0, betas=(momentum, 0.999)), `optimizer="sgd"` =
    SGD(param_groups(model, weight_decay), lr0, momentum, nesterov=True) -- three groups, the decay on the convolution weights only;
    `branch_weight=True` weights the heads' losses by train_params["branch_weight"] (train_step).  The defaults (None, False) read none of
    the three: the reference's Adam on one group, the heads summed unweighted.  The warm-up and the cosine schedule are the reference's in
    every case (yolov5's momentum / bias-lr warm-up is not part of this).
    `ema=True`, opt-in like these: yolov5's ModelEMA(model), built once the weights are loaded or initialised and updated by every
    train_step (inside the optimizer's launch); from epoch 5 on validation runs on `ema.ema`, as yolov5 validates its average, and a
    `YOLO-Fastest_epoch_N_ema.pth` with the average's state-dict (loadable like the other) is written beside each
    `YOLO-Fastest_epoch_N.pth`, which stays the raw model's.  With several ranks sync_buffers runs on `ema.ema` too -- the gradients are
    averaged, so the ranks' parameter averages agree, but their running statistics do not; that path needs more than one GPU and has
    not been run.  With ema=False nothing of this is constructed or read.
    `box_loss="giou" | "diou" | "ciou"`, opt-in like these: both heads regress the box of a positive cell as one IoU-family term in place
    of the reference's four coordinate terms, total = lambda_box * box + conf + cls (validation.YOLOLossV3; yf_train_head_loss_box).
    lambda_box = 5.0 is the sum of the reference's weights on x, y and on w, h; nobody has trained with it.  tbwriter then gets the
    scalar `box` in place of `x`, and no `y`, `w`, `h`.  It composes with branch_weight and ema (train_step is unchanged).  The decode
    stays the reference's, so the checkpoints load into detect.py as before.
    `loss_hyp`, opt-in like these: a dict with the loss keys of yolov5's hyp files -- `obj`, `cls`, `obj_pw`, `cls_pw`, `fl_gamma`,
    `label_smoothing`, plus `gr` (yolov5's model.gr) and `fl_alpha` -- handed to both heads' YOLOLossV3 (yf_train_head_loss_hyp;
    include/yolo_fastest_hip.h states the definition).  `obj` and `cls` are PLAIN gains on conf and cls in the total: they are not
    rescaled by the class count or the image size as yolov5's train.py rescales its own.  A missing key keeps its neutral value; an unknown
    key, a value the entry refuses, or gr > 0 without box_loss raises ValueError.  None (the default) constructs the loss objects as
    before.  yolov5's files use fl_gamma 0 or 1.5 and gr 1; no values are recommended, and nothing here has been trained with any of
    them.  It composes with branch_weight, ema, optimizer and box_loss (train_step is unchanged); the decode is untouched.
    `val_metrics=True`, opt-in like these: on the epochs where get_mAP runs, Validation.get_metrics (yolov5's P, R, mAP@.5, mAP@.5:.95 at
    conf_thres 0.001) runs right behind it on the same model (`ema.ema` with ema=True) and logs its table; tbwriter gets
    `metrics/precision`, `metrics/recall`, `metrics/mAP_0.5` and `metrics/mAP_0.5:0.95` per epoch, and rank 0 writes the validated model's
    state-dict to `YOLO-Fastest_best.pth` whenever the fitness (0.1 mAP@.5 + 0.9 mAP@.5:.95) strictly improves.  With False none of it runs.
    `val_nms` is get_metrics' `nms` ("reference", the default, or "yolov5": the detections get_metrics scores come from yolov5's own NMS,
    yf_val_nms_v5); it needs val_metrics=True, anything else with it raises ValueError.  get_mAP is the reference's either way.
    `autoanchor=True`, opt-in like these: yolov5's check_anchors (anchors.check_anchors, thr 4.0) runs on `train_dataset` before the
    losses are built -- on every rank, which must therefore share numpy's and `random`'s seeds -- and the io_params it returns (the
    configured anchors if their best possible recall is above 0.98, else anchors fitted on the device, if they recall more) are used for
    the losses and for Validation; the caller's `params` is not modified.  Rank 0 writes them as `YOLO-Fastest_anchors.json`
    ({"anchors": [[[w, h], ...] per head], "strides": [...]}) into save_path.  The checkpoint is a plain state-dict and carries NO
    anchors: whoever decodes with it (detect.py's io_params, YOLO_post_process) must put the written anchors into io_params["anchors"],
    or the boxes are decoded against the wrong shapes.  With False the `anchors` module is not imported.
    Returns the trained model."""
    import logging
    import os
    import time
    import numpy as np
    from torch.optim import lr_scheduler
    from torch.utils.data import DataLoader
    from . import validation
    from .model import YoloFastest
    if train_dataset is None:
        raise ValueError("pass train_dataset (e.g. dataset.DetectDataset over a Pascal-VOC tree, as train.py:68-76 builds it)")
    logger = logger or logging.getLogger(__name__)
    io, tp = params["io_params"], params["train_params"]
    if optimizer not in (None, "adam", "sgd"):
        raise ValueError("optimizer must be None (the reference's Adam), \"adam\" or \"sgd\", got %r" % (optimizer,))
    if val_nms not in validation.NMS_KINDS:
        raise ValueError("val_nms must be 'reference' or 'yolov5', not %r" % (val_nms,))
    if val_nms != "reference" and not val_metrics:
        raise ValueError("val_nms=%r is read by get_metrics only: pass val_metrics=True" % (val_nms,))
    hyp_kwargs = {}
    if loss_hyp is not None:
        unknown = sorted(set(loss_hyp) - set(LOSS_HYP_KEYS))
        if unknown:
            raise ValueError("loss_hyp: unknown key(s) %s; known: %s" % (", ".join(map(repr, unknown)), ", ".join(LOSS_HYP_KEYS)))
        hyp_kwargs = {LOSS_HYP_KEYS[k]: float(v) for k, v in loss_hyp.items()}
        if hyp_kwargs.get("obj_iou", 0.0) > 0 and box_loss is None:
            raise ValueError("loss_hyp['gr'] > 0 needs box_loss: the reference's four coordinate terms have no IoU value")
        validation.YOLOLossV3(anchors=io["anchors"][0], num_classes=io["num_cls"], input_shape=io["input_shape"], device=device,
                              box_loss=box_loss, lambda_box=lambda_box, **hyp_kwargs)       # every other refusal, before anything is built
    head_weights = None
    if branch_weight:
        head_weights = [float(v) for v in tp["branch_weight"]]
        if len(head_weights) != len(io["strides"]):
            raise ValueError("train_params['branch_weight'] has %d entries, io_params['strides'] %d" % (len(head_weights), len(io["strides"])))
    save_path = io["save_path"]
    os.makedirs(save_path, exist_ok=True)
    if autoanchor:
        import json
        import torch.distributed as tdist
        from . import anchors as autoanchors
        io = autoanchors.check_anchors(train_dataset, io, thr=4.0, logger=logger, device=device)
        params = dict(params, io_params=io)                   # Validation reads params["io_params"]; the caller's dict stays as it was
        if not tdist.is_initialized() or tdist.get_rank() == 0:
            with open(os.path.join(save_path, "YOLO-Fastest_anchors.json"), "w") as f:
                json.dump({"anchors": io["anchors"], "strides": list(io["strides"])}, f)
    total_epochs, batch_size = tp["total_epochs"], tp["batch_size"]
    model = YoloFastest(io).to(device)
    model_loss = [validation.YOLOLossV3(anchors=io["anchors"][i], num_classes=io["num_cls"], input_shape=io["input_shape"], device=device,
                                        model=model, box_loss=box_loss, lambda_box=lambda_box, **hyp_kwargs) for i in range(len(io["strides"]))]
    for ml in model_loss:
        ml.ignore_threshold = tp.get("IOU_loss_thre", 0.5)
    if tp.get("pretrained_pth") and os.path.exists(tp["pretrained_pth"]):
        logger.info("Load pretrained model %s" % tp["pretrained_pth"])
        model.load_state_dict(torch.load(tp["pretrained_pth"], map_location=device))
    else:
        logger.info("initialize model")
        model.initialize_weights()
    import torch.distributed as tdist
    world = tdist.get_world_size() if tdist.is_initialized() else 1
    rank = tdist.get_rank() if tdist.is_initialized() else 0
    sampler = None
    if world > 1:            # one process per GPU: every rank its own shard of each epoch, gradients averaged by data_parallel()
        from torch.utils.data.distributed import DistributedSampler
        sampler = DistributedSampler(train_dataset, num_replicas=world, rank=rank, shuffle=True, drop_last=True)
        data_parallel(model)
    model_ema = ModelEMA(model) if ema else None             # (behind data_parallel's broadcast: every rank averages rank 0's start)
    dataloader = DataLoader(train_dataset, batch_size=batch_size, num_workers=0, drop_last=True, pin_memory=True, shuffle=sampler is None,
                            sampler=sampler, collate_fn=validation.collate_fn)
    val = validation.Validation(params=params, logger=logger, dataset=val_dataset, device=device, model_loss=model_loss,
                                match=val_match) if val_dataset is not None else None
    batch_per_epoch = len(dataloader)
    num_warm = max(3 * batch_per_epoch, 1000)
    if optimizer is None:
        optimizer = Adam(model.parameters(), lr=tp["lr0"], betas=(0.9, 0.999), eps=1e-08)
    elif optimizer == "adam":
        optimizer = Adam(param_groups(model, tp["weight_decay"]), lr=tp["lr0"], betas=(tp["momentum"], 0.999), eps=1e-08)
    else:
        optimizer = SGD(param_groups(model, tp["weight_decay"]), lr=tp["lr0"], momentum=tp["momentum"], nesterov=True)

    def lf(epoch):
        return cosine_factor(epoch, total_epochs)
    scheduler = lr_scheduler.LambdaLR(optimizer, lr_lambda=lf)
    start_epoch = 0
    best_fitness = float("-inf")                              # (val_metrics) the first validated epoch always improves on it
    scheduler.last_epoch = start_epoch - 1
    total_steps = (total_epochs - start_epoch) * batch_per_epoch
    step_count = 0
    logger.info("Start training.")
    losses_name = ["total_loss", "x", "y", "w", "h", "conf", "cls"]
    if box_loss is not None:
        losses_name = ["total_loss", "box", None, None, None, "conf", "cls"]     # [2..4] are zeros then
    for epoch in range(start_epoch, total_epochs):
        model.train()
        if sampler is not None:
            sampler.set_epoch(epoch)
        for batch_id, (imgs, targets) in enumerate(dataloader):
            start_time = time.time()
            imgs = imgs.to(device).float()
            targets = targets.to(device).float()
            iteration = batch_id + batch_per_epoch * epoch
            if iteration <= num_warm:
                for x in optimizer.param_groups:
                    x["lr"] = np.interp(iteration, [0, num_warm], [0.0, x["initial_lr"] * lf(epoch)])
            if model_ema is not None:
                losses = train_step(model, model_loss, optimizer, imgs, targets, head_weights, ema=model_ema)
            elif head_weights is None:
                losses = train_step(model, model_loss, optimizer, imgs, targets)
            else:
                losses = train_step(model, model_loss, optimizer, imgs, targets, head_weights)
            step_count += 1
            if step_count > 0 and step_count % 10 == 0:
                _loss = losses[0].item()
                duration = float(time.time() - start_time)
                example_per_second = batch_size / duration
                _remain = (total_steps - step_count) * duration
                _m, _s = divmod(_remain, 60)
                _h, _m = divmod(_m, 60)
                lr = optimizer.param_groups[0]["lr"]
                logger.info("epoch [%d]: current_batch = %d/%d, total_iter = %d, loss = %.5f, example/sec = %.3f, lr = %.5f, remain = %d:%02d:%02d" %
                            (epoch, batch_id + 1, batch_per_epoch, step_count, _loss, example_per_second, lr, _h, _m, _s))
                if tbwriter is not None:
                    tbwriter.add_scalar("lr", lr, step_count)
                    tbwriter.add_scalar("example/sec", example_per_second, step_count)
                    for i, name in enumerate(losses_name):
                        if name is None:
                            continue
                        tbwriter.add_scalar(name, _loss if i == 0 else losses[i], step_count)
        scheduler.step()
        if world > 1:
            sync_buffers(model)                      # validation and the checkpoint see rank 0's running statistics on every rank
            if model_ema is not None:
                sync_buffers(model_ema.ema)
                model_ema.ema._weights_dirty = True
        if epoch > 4 and val is not None:
            validated = model if model_ema is None else model_ema.ema
            val.get_mAP(epoch=epoch, model=validated)
            if val_metrics:
                scores = val.get_metrics(model=validated, epoch=epoch, nms=val_nms)
                if tbwriter is not None:
                    for name, key in (("precision", "precision"), ("recall", "recall"), ("mAP_0.5", "mAP50"), ("mAP_0.5:0.95", "mAP50_95")):
                        tbwriter.add_scalar("metrics/" + name, scores[key], epoch)
                if rank == 0 and scores["fitness"] > best_fitness:
                    best_fitness = scores["fitness"]
                    torch.save(validated.state_dict(), os.path.join(save_path, "YOLO-Fastest_best.pth"))
        if rank == 0:
            torch.save(model.state_dict(), os.path.join(save_path, "YOLO-Fastest_epoch_{}.pth".format(str(epoch))))
            if model_ema is not None:
                torch.save(model_ema.ema.state_dict(), os.path.join(save_path, "YOLO-Fastest_epoch_{}_ema.pth".format(str(epoch))))
    return model
