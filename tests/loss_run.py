"""The one runner of the three training-loss entries for tests/test_gpu_loss.py ("ex": yf_train_head_loss_ex, 6 + C planes),
tests/test_gpu_box_loss.py ("box": yf_train_head_loss_box, 8 + C planes) and tests/test_gpu_loss_hyp.py ("hyp": yf_train_head_loss_hyp,
8 + C planes), called through ctypes: the workspace is exactly the reported size; it, d_losses[8] and d_grad_head each sit between two
4 KiB guards of 0xA5 bytes that must come back untouched; the gradient is pre-filled with a NaN pattern and must come back fully written;
the reserved bytes behind the planes must come back unwritten."""
import collections
import ctypes

import numpy as np
import torch

import loss_cases as lc

GUARD = 4096
NAN_BITS = 0x7FC0A5A5          # a quiet NaN no kernel computes

Entry = collections.namedtuple("Entry", "size loss planes")            # the planes on top of the C class planes
ENTRIES = {"ex": Entry("yf_train_head_loss_workspace_bytes_ex", "yf_train_head_loss_ex", 6),
           "box": Entry("yf_train_head_loss_box_workspace_bytes", "yf_train_head_loss_box", 8),
           "hyp": Entry("yf_train_head_loss_hyp_workspace_bytes", "yf_train_head_loss_hyp", 8)}


class Guarded:
    """`nbytes` of device memory between two 4 KiB guards, everything 0xA5"""

    def __init__(self, nbytes, dev):
        self.nbytes = nbytes
        self.buf = torch.full((GUARD + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        self.ptr = self.buf.data_ptr() + GUARD
        assert self.ptr % 8 == 0

    def payload(self):
        return self.buf[GUARD:GUARD + self.nbytes].cpu().numpy()

    def guards_untouched(self):
        return bool((self.buf[:GUARD] == 0xA5).all()) and bool((self.buf[GUARD + self.nbytes:] == 0xA5).all())


def need(lib, c, entry):
    """the entry's workspace size for case c, held to the layout the header states; "hyp" reports exactly the box entry's"""
    n = ctypes.c_size_t()
    assert getattr(lib, ENTRIES[entry].size)(c.N, c.fh, c.fw, c.A, c.C, ctypes.byref(n)) == 0
    E = c.N * c.A * c.fh * c.fw
    planes = ENTRIES[entry].planes + c.C
    assert 16 * 8 + planes * E * 4 <= n.value <= 16 * 8 + planes * E * 4 + 64
    if entry == "hyp":
        assert n.value == need(lib, c, "box")
    return n.value


def anc(c):
    return (ctypes.c_double * (2 * c.A))(*[float(v) for a in c.anchors for v in a])


def call(lib, entry, c, x, t, work_ptr, nbytes, losses_ptr, grad_ptr, stream, kind=0, lam=0.0, opts=None, A=None, C=None, T=None, anchors=None):
    """the entry's return code.  kind, lam: box_kind and lambda_box ("box", "hyp"); opts: the eight options in the entry's order ("hyp");
    A, C, T, anchors: in place of the case's own (the refusals)"""
    tail = {"ex": (), "box": (kind, lam), "hyp": (kind, lam) + tuple(opts or ())}[entry]
    return getattr(lib, ENTRIES[entry].loss)(0, c.H, c.W, x.data_ptr(), c.N, c.fh, c.fw, anc(c) if anchors is None else anchors,
                                             c.A if A is None else A, c.C if C is None else C, t.data_ptr(), c.T if T is None else T, lc.THRES,
                                             work_ptr, nbytes, losses_ptr, grad_ptr, stream, *tail)


def run(lib, dev, c, entry, kind=0, lam=0.0, opts=None, grad=True, stream=None):
    """-> (losses float32 [8], grad float32 like the logits or None, dense float32 [6 + C or 8 + C, E], acc float64 [16]); asserts the
    guards"""
    E = c.N * c.A * c.fh * c.fw
    planes = ENTRIES[entry].planes + c.C
    nbytes = need(lib, c, entry)
    x = torch.from_numpy(c.logits).to(dev)
    t = torch.from_numpy(c.targets).to(dev)
    work, losses = Guarded(nbytes, dev), Guarded(8 * 4, dev)
    g = Guarded(c.logits.size * 4, dev) if grad else None
    if grad:
        g.buf[GUARD:GUARD + g.nbytes].view(torch.int32).fill_(NAN_BITS)
    torch.cuda.synchronize(dev)
    s = ctypes.c_void_p(stream.cuda_stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream)
    rc = call(lib, entry, c, x, t, work.ptr, nbytes, losses.ptr, g.ptr if grad else None, s, kind, lam, opts)
    assert rc == 0, lib.yf_last_error_string()
    torch.cuda.synchronize(dev)
    for what, b in (("workspace", work), ("losses", losses), ("gradient", g)):
        assert b is None or b.guards_untouched(), (c.name, what)
    w = work.payload()
    acc = w[:128].view(np.float64).copy()
    dense = w[128:128 + planes * E * 4].view(np.float32).reshape(planes, E).copy()
    assert (w[128 + planes * E * 4:] == 0xA5).all(), (c.name, "the reserved bytes behind the planes were written")
    l8 = losses.payload().view(np.float32).copy()
    gh = None
    if grad:
        gh = g.payload().view(np.float32).copy()
        assert not (gh.view(np.int32) == np.int32(NAN_BITS)).any(), (c.name, "gradient elements left unwritten")
        gh = gh.reshape(c.logits.shape)
    return l8, gh, dense, acc
