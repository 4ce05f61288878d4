"""Baseline and, opt-in, progressive JPEG files decoded on the device (csrc/yf_jpeg_kernels.hip): the bytes `cv2.imread` would return, exactly what
`np.asarray(PIL.Image.open(path).convert("RGB"))[:, :, ::-1]` gives (libjpeg-turbo's ISLOW IDCT, fancy upsampling and integer colour
tables, restated bit for bit), as uint8 device tensors [n, h, w, 3] in BGR order.

Supported: SOF0 / SOF1, 8-bit, Huffman coding, 1 component (gray: the value in all three bytes) or 3 (YCbCr or RGB as libjpeg guesses it;
luma sampling 1 or 2 each way, chroma 1 x 1: 4:4:4, 4:2:2, 4:2:0, 4:4:0), restart markers, custom tables, up to 8192 x 8192.  Anything
else is refused on the host with a ValueError naming the file (there is no fallback here: the caller picks PIL instead).  Corrupt or
truncated entropy data raises OSError naming the file, as PIL does for truncated files.  No EXIF orientation is applied (PIL does not
apply it either).

`progressive=True` (frame_size, pack, decode_files) also takes SOF2 files: 8-bit, Huffman, the same layouts, at most 256 scans, and a
complete progression (every coefficient coded down to Al = 0; libjpeg smooths the blocks of an incomplete one, so such a file is
refused).  Baseline files decode to the same bytes through the same kernels with or without the flag.  It is opt-in because a progressive
frame costs more device time than its baseline twin: its scans are serial chains."""
import ctypes
import os
from typing import List, NamedTuple

import torch

from . import _lib


class JpegGroup(NamedTuple):
    """The frames of one size: `bgr` uint8 device [len(positions), h, w, 3]; `positions` their indices in the call's input list."""
    positions: List[int]
    bgr: torch.Tensor


def check_decode(decode, progressive):
    """The `decode` / `progressive` keywords of the drivers that start from image files (DetectDataset, Detect_YOLO)."""
    if decode not in ("host", "device"):
        raise ValueError('decode must be "host" or "device"')
    if progressive and decode != "device":
        raise ValueError('progressive=True needs decode="device" (PIL, the host decoder, reads progressive files anyway)')


def cuda_device(device):
    """torch.device(device); "cuda" without an index means the current device."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def _name(item, i):
    return item if isinstance(item, (str, os.PathLike)) else "<bytes #%d>" % i


def _bytes(item):
    if isinstance(item, (bytes, bytearray, memoryview)):
        return bytes(item)
    with open(item, "rb") as f:
        return f.read()


def _pack_call(datas, blob_ptr, blob_cap, progressive=False):
    n = len(datas)
    ptrs = (ctypes.c_void_p * n)(*[ctypes.cast(ctypes.c_char_p(d), ctypes.c_void_p) for d in datas])
    sizes = (ctypes.c_size_t * n)(*[len(d) for d in datas])
    need, h, w = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_int()
    rc = _lib.lib().yf_jpeg_pack_ex(n, ptrs, sizes, _lib.YF_JPEG_PROGRESSIVE if progressive else 0, blob_ptr, blob_cap, ctypes.byref(need),
                                    ctypes.byref(h), ctypes.byref(w))
    return rc, need.value, h.value, w.value


def _refusal(rc, names):
    msg = _lib.lib().yf_last_error_string().decode(errors="replace")
    if rc == _lib.YF_E_INVALID and msg.startswith("frame "):
        head, _, reason = msg.partition(": ")
        i = int(head.split()[1])
        return ValueError("%s: %s" % (names[i], reason))
    return _lib.YFError("yolo_fastest_hip error %d: %s" % (rc, msg))


def frame_size(data, name="<bytes>", progressive=False):
    """(h, w) of one JPEG file's bytes; ValueError if the device decoder does not support it (progressive files: only with
    `progressive=True`)."""
    rc, _, h, w = _pack_call([data], None, 0, progressive)
    if rc:
        raise _refusal(rc, [name])
    return h, w


def pack(datas, names=None, pin=True, progressive=False):
    """The host blob of frames of one size (yf_jpeg_pack_ex, flags 0 or YF_JPEG_PROGRESSIVE) in a (pinned) uint8 CPU tensor
    -> (blob, h, w)."""
    names = names or ["<bytes #%d>" % i for i in range(len(datas))]
    rc, need, h, w = _pack_call(datas, None, 0, progressive)
    if rc:
        raise _refusal(rc, names)
    blob = torch.empty(need, dtype=torch.uint8, pin_memory=pin)
    rc, _, _, _ = _pack_call(datas, ctypes.c_void_p(blob.data_ptr()), need, progressive)
    if rc:
        raise _refusal(rc, names)
    return blob, h, w


def workspace_bytes(blob):
    n = ctypes.c_size_t()
    _lib.check(_lib.lib().yf_jpeg_workspace_bytes(ctypes.c_void_p(blob.data_ptr()), ctypes.byref(n)))
    return n.value


def decode_blob(blob, h, w, device, out=None, status=None, workspace=None):
    """Stream-ordered decode of a packed blob on `device` (current stream): uploads it without blocking, launches, returns
    (bgr uint8 [n, h, w, 3], status int32 [n]) without synchronising.  The pinned `blob` must outlive the upload."""
    device = torch.device(device)
    n = ctypes.cast(blob.data_ptr(), ctypes.POINTER(ctypes.c_int32))[1]
    stream = torch.cuda.current_stream(device)
    d_blob = torch.empty(blob.numel(), dtype=torch.uint8, device=device)
    d_blob.copy_(blob, non_blocking=True)
    ws_bytes = workspace_bytes(blob)
    if workspace is None:
        workspace = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=device)
    if out is None:
        out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=device)
    if status is None:
        status = torch.empty((n,), dtype=torch.int32, device=device)
    _lib.check(_lib.lib().yf_jpeg_decode_u8(device.index, ctypes.c_void_p(blob.data_ptr()), ctypes.c_void_p(d_blob.data_ptr()),
                                            ctypes.c_void_p(workspace.data_ptr()), workspace.numel(), ctypes.c_void_p(out.data_ptr()),
                                            ctypes.c_void_p(status.data_ptr()), ctypes.c_void_p(stream.cuda_stream)))
    return out, status


def scan_info(blob, frame=0, scan=0):
    """yf_jpeg_scan_info as a dict: scans and levels of the frame (scans 0: a baseline frame) and scan `scan` (file order)."""
    a = (ctypes.c_int * 12)()
    _lib.check(_lib.lib().yf_jpeg_scan_info(ctypes.c_void_p(blob.data_ptr()), frame, scan, a, 12))
    keys = ("scans", "levels", "ncomp", "comp_mask", "ss", "se", "ah", "al", "level", "offset", "length", "ri")
    return dict(zip(keys, a))


def decode_files(paths_or_bytes, device, progressive=False):
    """Paths and / or bytes of JPEG files -> [JpegGroup(positions, bgr uint8 device [n_g, h, w, 3])], one group per frame size in order
    of first appearance, one decode call per group.  Raises ValueError (unsupported file) before any launch and OSError (corrupt or
    truncated data) after checking the status words.  `progressive=True`: progressive files are decoded too (a size's group may mix
    kinds); without it they are refused."""
    device = cuda_device(device)
    if device.type != "cuda":
        raise RuntimeError("JPEG decoding on the device needs a cuda device")
    items = list(paths_or_bytes)
    datas = [_bytes(x) for x in items]
    names = [_name(x, i) for i, x in enumerate(items)]
    order = {}
    for i, d in enumerate(datas):
        order.setdefault(frame_size(d, names[i], progressive), []).append(i)
    groups, statuses, keep = [], [], []
    for (h, w), pos in order.items():
        blob, _, _ = pack([datas[i] for i in pos], [names[i] for i in pos], progressive=progressive)
        bgr, st = decode_blob(blob, h, w, device)
        groups.append(JpegGroup(pos, bgr))
        statuses.append(st)
        keep.append(blob)
    if groups:
        st = torch.cat(statuses).cpu()            # waits for the launches (and so for the pinned blobs' uploads)
        flat = [i for g in groups for i in g.positions]
        bad = [(flat[k], int(st[k])) for k in range(len(flat)) if int(st[k]) != 0]
        if bad:
            i, s = bad[0]
            raise OSError("%s: corrupt or truncated JPEG data (decoder status 0x%x)%s"
                          % (names[i], s, "" if len(bad) == 1 else "; %d more such files in this call" % (len(bad) - 1)))
    del keep
    return groups


def frames_in_order(groups, stacks=None):
    """decode_files' groups back in the order of its input: the [n, h, w, 3] stack itself when there is one group, else a list of
    [h, w, 3] views.  `stacks`: one [n_g, h, w, 3] array per group to take the frames from in place of `bgr` (the groups' host copies)."""
    stacks = [g.bgr for g in groups] if stacks is None else stacks
    if len(groups) == 1:
        return stacks[0]
    frames = [None] * sum(len(g.positions) for g in groups)
    for g, stack in zip(groups, stacks):
        for k, p in enumerate(g.positions):
            frames[p] = stack[k]
    return frames


# ---- encoding (csrc/yf_jpeg_enc_kernels.hip): byte for byte the file PIL writes for Image.save(f, "JPEG", quality=q, subsampling=s) ----

_SUBSAMPLING = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}


class EncSetup(NamedTuple):
    """yf_jpeg_enc_setup's blob (a uint8 CPU tensor) and what it holds: the file header, the divisors 8 * q and their reciprocals per
    table ([luma, chroma], natural order), and blocks per frame."""
    blob: torch.Tensor
    header: bytes
    divisors: list
    reciprocals: list
    blocks: int


def enc_setup(h, w, channels, quality=95, subsampling="4:2:0"):
    """Host only.  ValueError for what the device encoder does not build: channels other than 1 or 3, quality outside 1..100, other
    subsampling strings, sides above 8192, frames whose worst-case stream exceeds 2^31 bits."""
    if subsampling not in _SUBSAMPLING:
        raise ValueError('subsampling must be "4:4:4", "4:2:2" or "4:2:0", got %r' % (subsampling,))
    if isinstance(quality, bool) or not isinstance(quality, int):
        raise ValueError("quality must be an int 1..100, got %r" % (quality,))
    lib = _lib.lib()
    need = ctypes.c_size_t()
    args = (int(h), int(w), int(channels), quality, _SUBSAMPLING[subsampling])
    rc = lib.yf_jpeg_enc_setup(*args, None, 0, ctypes.byref(need))
    if rc == _lib.YF_E_INVALID:
        raise ValueError(lib.yf_last_error_string().decode(errors="replace"))
    _lib.check(rc)
    blob = torch.empty(need.value, dtype=torch.uint8)
    _lib.check(lib.yf_jpeg_enc_setup(*args, ctypes.c_void_p(blob.data_ptr()), need.value, ctypes.byref(need)))
    info = (ctypes.c_int * 10)()
    header = ctypes.create_string_buffer(640)
    div, rcp = (ctypes.c_uint16 * 128)(), (ctypes.c_uint32 * 128)()
    _lib.check(lib.yf_jpeg_enc_info(ctypes.c_void_p(blob.data_ptr()), info, 10, header, div, rcp))
    return EncSetup(blob, header.raw[:info[6]], [list(div[:64]), list(div[64:])], [list(rcp[:64]), list(rcp[64:])], info[7])


def enc_workspace_bytes(setup, n):
    """Device workspace encode_batch needs for n frames of `setup`."""
    need = ctypes.c_size_t()
    _lib.check(_lib.lib().yf_jpeg_enc_workspace_bytes(ctypes.c_void_p(setup.blob.data_ptr()), n, ctypes.byref(need)))
    return need.value


def _enc_check(frames, quality, subsampling, order, optimize, progressive):
    if optimize or progressive:
        raise ValueError("the device encoder writes baseline files with the Annex K tables: optimize / progressive are not built")
    if order not in ("bgr", "rgb"):
        raise ValueError('order must be "bgr" or "rgb"')
    if not torch.is_tensor(frames) or not frames.is_cuda or frames.dtype != torch.uint8:
        raise ValueError("expected a uint8 GPU tensor [n, h, w, 3] or [n, h, w]")
    if frames.dim() not in (3, 4) or (frames.dim() == 4 and frames.shape[3] != 3) or frames.shape[0] < 1:
        raise ValueError("expected a uint8 GPU tensor [n, h, w, 3] or [n, h, w] with n >= 1, got %s" % (tuple(frames.shape),))
    return enc_setup(frames.shape[1], frames.shape[2], 3 if frames.dim() == 4 else 1, quality, subsampling)


def encode_batch(frames, quality=95, subsampling="4:2:0", order="bgr", stride=None, optimize=False, progressive=False, setup=None,
                 workspace=None, out=None, lengths=None, status=None):
    """Stream-ordered (current stream), nothing synchronises: uint8 device frames [n, h, w, 3] (`order` "bgr" as decode_files hands them
    out, or "rgb") or [n, h, w] (gray) -> (buffer uint8 [n, stride], lengths int32 [n], status int32 [n]) on the device.  Frame f's file is
    buffer[f, :lengths[f]]; status[f] = 1 means it did not fit `stride` (default h * w * channels + 1024) and lengths[f] is the stride it
    needs.  Capturable when `workspace`, `out`, `lengths` and `status` are passed in (allocated before the capture)."""
    s = setup or _enc_check(frames, quality, subsampling, order, optimize, progressive)
    frames = frames.contiguous()
    n = frames.shape[0]
    dev = frames.device
    if stride is None:
        stride = frames[0].numel() + 1024
    lib = _lib.lib()
    if workspace is None:
        workspace = torch.empty(enc_workspace_bytes(s, n), dtype=torch.uint8, device=dev)
    if out is None:
        out = torch.empty((n, stride), dtype=torch.uint8, device=dev)
    if lengths is None:
        lengths = torch.empty((n,), dtype=torch.int32, device=dev)
    if status is None:
        status = torch.empty((n,), dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev)
    _lib.check(lib.yf_jpeg_encode_u8(dev.index, ctypes.c_void_p(s.blob.data_ptr()), ctypes.c_void_p(frames.data_ptr()), n, int(order == "bgr"),
                                     ctypes.c_void_p(workspace.data_ptr()), workspace.numel(), ctypes.c_void_p(out.data_ptr()), out.shape[1],
                                     ctypes.c_void_p(lengths.data_ptr()), ctypes.c_void_p(status.data_ptr()), ctypes.c_void_p(stream.cuda_stream)))
    return out, lengths, status


def gather_files(out, lengths):
    """(buffer [n, stride] on the device, lengths as a host list) -> [bytes]: one device-to-host copy of the used part of the buffer."""
    most = max(lengths)
    host = out[:, :most].cpu().numpy()
    return [host[f, :lengths[f]].tobytes() for f in range(len(lengths))]


def gather_encoded(frames, out, lengths, status, quality=95, subsampling="4:2:0", order="bgr"):
    """encode_batch's `out` for `frames`, with its `lengths` and `status` as host lists -> [bytes], one complete file per frame.  Frames
    that outgrew `out`'s stride are encoded once more with the size they need (the kernels report it); there is no host fallback."""
    over = [f for f in range(len(status)) if status[f]]
    fit = [f for f in range(len(status)) if not status[f]]
    files = [None] * len(status)
    if fit:
        for f, d in zip(fit, gather_files(out[fit] if over else out, [lengths[f] for f in fit])):
            files[f] = d
    if over:
        out2, l2, s2 = encode_batch(frames[over], quality, subsampling, order, stride=max(lengths[f] for f in over))
        l2, s2 = torch.stack([l2, s2]).cpu().tolist()
        if any(s2):
            raise _lib.YFError("the device JPEG encoder overflowed the size it asked for")
        for f, d in zip(over, gather_files(out2, l2)):
            files[f] = d
    return files


def encode_frames(frames, quality=95, subsampling="4:2:0", order="bgr", stride=None, optimize=False, progressive=False):
    """uint8 device frames -> [bytes], one complete JPEG file per frame: what PIL writes for `Image.fromarray(rgb_or_gray).save(f, "JPEG",
    quality=quality, subsampling=subsampling)` (gather_encoded after one encode_batch)."""
    out, lengths, status = encode_batch(frames, quality, subsampling, order, stride, optimize, progressive)
    lengths, status = torch.stack([lengths, status]).cpu().tolist()
    return gather_encoded(frames, out, lengths, status, quality, subsampling, order)
