"""The inference engine on poisoned, guarded memory (tests/arena.py): a result is a function of its tensors alone, and every write stays
inside the sizes the ABI reports.

The C entry points are called directly, as `model.forward` calls them, with EVERY caller-owned buffer -- input, both heads, the workspace of
exactly `yf_workspace_bytes`, the record block -- carved out of one arena that is pre-filled with 0x00, with 0xFF (NaN as fp32 and fp16) and
with a byte ramp.  Several hot kernels read out of bounds on purpose (k19's region loads into the workspace guard band, the block kernels'
repeated last tile, the stem's halo): that is correct only if what they read is dropped by a select.  `0 * garbage` gives the right answer
on the finite leftovers of `torch.empty` and NaN on 0xFF -- which the next ReLU turns into 0: on the device a poisoned operand shows as a
finite wrong value, so (d) and (e) carry the weight (shown once with a planted fault in the stem: DESIGN.md).  Under each fill: (a) the guards are intact, (b) the input is unchanged, (c) both
heads are fully written and finite, (d) bitwise equal across the fills, (e) bitwise equal to `model(x)`.

Cases: the smallest shapes that reach every launch form (SHAPES below) in the precision x fusion product of tests/replay.py's cases;
`test_every_launch_form_is_poisoned` holds the union of (kind, form) to theirs with the device's CU count.  Then the u8 / BGR entries (the
net-sized u8 frames sit at the workspace's tail), two lanes, the packed post-process, and a NaN frame between two clean ones."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import backbone_oracle as bo
from tests import arena as ar
from tests import replay as rp

pytestmark = pytest.mark.gpu
rp.cap_threads()

# The shapes, written out on their own (not derived from replay's tables): 96x160, 160x224, 256x352 and 256x320 at N=2; 256x320 at the
# split-sum threshold and one frame past it; the two large batches that leave the few-frames tilings.  Precisions f32, f16x3, f16; fusion
# 1 and 2, plus 0 for f32 -- test_every_launch_form_is_poisoned holds the forms this product reaches to those of replay's cases.
SHAPES = [(96, 160, 2), (160, 224, 2), (256, 352, 2), (256, 320, 2), (256, 320, rp.ESPLIT_MAX_FRAMES), (256, 320, rp.ESPLIT_MAX_FRAMES + 1),
          (96, 160, 132), (160, 224, 36)]
CASES = [(p, f, c) for c in SHAPES for p in ("f32", "f16x3", "f16") for f in ((0, 1, 2) if p == "f32" else (1, 2))]

def _ID(v):
    return ("%dx%d-N%d" if len(v) == 3 else "%dx%d") % v if isinstance(v, tuple) else str(v)


@pytest.fixture(scope="module")
def yf():
    import yolo_fastest_amd
    return yolo_fastest_amd


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def models(yf, dev):
    out = {}
    for k, load in rp.state_dicts().items():
        m = yf.YoloFastest(yf.io_params_for(256)).to(dev).eval()
        m.load_state_dict(load())
        out[k] = m
    return out


class _Knobs:
    """model.precision / .fusion / .chunk / .lanes for the length of a case."""

    def __init__(self, yf, m, precision=None, fusion=None, chunk=0, lanes=2):
        self.yf, self.m, self.set = yf, m, (precision, yf.model.DEFAULT_FUSION if fusion is None else fusion, chunk, lanes)

    def __enter__(self):
        self.m.precision, self.m.fusion, self.m.chunk, self.m.lanes = self.set

    def __exit__(self, *a):
        self.m.precision, self.m.fusion, self.m.chunk, self.m.lanes = None, self.yf.model.DEFAULT_FUSION, 0, 2


def _ws_bytes(yf, e, N):
    need = ctypes.c_size_t()
    yf._lib.check(e.lib.yf_workspace_bytes(e.handle, N, ctypes.byref(need)))
    return need.value


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _poisoned(yf, m, dev, src, H, W, call, want):
    """`call(e, src in the arena, hl, hs, ws, ws bytes)` under every fill, heads and workspace in the arena -> asserts (a) .. (e)."""
    N = src.shape[0]
    e = m.engine(H, W, N, dev)
    need = _ws_bytes(yf, e, N)
    shapes = ((N, m.num_out, H // 16, W // 16), (N, m.num_out, H // 32, W // 32))
    cap = ar.room([src.numel() * src.element_size()] + [4 * int(np.prod(s)) for s in shapes]) + ar.room([need], ar.WS_GUARD)

    def run(a):
        x = a.put(src, "input")
        hl, hs = a.empty(shapes[0], torch.float32, "head_large"), a.empty(shapes[1], torch.float32, "head_small")
        ws = a.take(need, "workspace", guard=ar.WS_GUARD)
        call(e, x, hl, hs, ws, need)
        return {"input": x, "head_large": hl, "head_small": hs}
    return ar.run_fills(dev, cap, run, {"input": src, "head_large": want[0], "head_small": want[1]})


def _forward(yf, dev):
    def call(e, x, hl, hs, ws, need):
        yf._lib.check(e.lib.yf_forward(e.handle, x.data_ptr(), x.shape[0], hl.data_ptr(), hs.data_ptr(), ws.data_ptr(), need, _stream(dev)))
    return call


def test_every_launch_form_is_poisoned(dev):
    """The union of (kind, form) over the poison cases is the union over replay's cases, with this device's CU count."""
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count

    def union(cases):
        return {(L.kind, L.form) for p, f, (H, W, N) in cases for L in rp.launch_table(H, W, f, p, N=N, n_cu=n_cu)}
    replayed = [(p, f, (H, W, N)) for H, W, N, fusions, precisions in rp.CASES_F32 for f in fusions for p in precisions] + \
               [("f16", f, c) for c in rp.CASES_F16 for f in (1, 2)]
    assert set(replayed) != set(CASES)                              # two lists of their own: the equality below is no tautology
    missing, extra = union(replayed) - union(CASES), union(CASES) - union(replayed)
    assert not missing and not extra, (sorted(missing), sorted(extra))
    for p, f, (H, W, N) in CASES:                                  # and each case reaches the forms replay's `expect` names for it
        if p != "f16":
            fm = rp.forms(rp.launch_table(H, W, f, p, N=N, n_cu=n_cu))
            for name, (kind, disp) in rp.expect(H, W, N, f, p, n_cu).items():
                assert fm[name][:2] == (kind, disp), (p, f, H, W, N, name, fm[name])


@pytest.mark.parametrize("precision,fusion,case", CASES, ids=_ID)
def test_forward_depends_on_its_tensors_alone(yf, models, golden, dev, precision, fusion, case):
    H, W, N = case
    m = models["random" if N > 30 else "shipped"]          # the large batches with the seeded random weights only, as replay.RANDOM_ONLY does
    x = bo.preprocess(rp.frames_u8(golden, H, W, N)).to(dev)
    with _Knobs(yf, m, precision, fusion), torch.no_grad():
        want = m(x)
        torch.cuda.synchronize(dev)
        _poisoned(yf, m, dev, x, H, W, _forward(yf, dev), want)


@pytest.mark.parametrize("size", [(256, 320), (512, 640)], ids=_ID)
def test_forward_u8_at_the_nets_size_and_twice_it(yf, models, dev, size):
    m = models["shipped"]
    u8 = torch.from_numpy(np.random.default_rng(size[0]).integers(0, 256, (2,) + size, dtype=np.uint8)).to(dev)

    def call(e, x, hl, hs, ws, need):
        yf._lib.check(e.lib.yf_forward_u8(e.handle, x.data_ptr(), 2, size[0], size[1], hl.data_ptr(), hs.data_ptr(), ws.data_ptr(), need, _stream(dev)))
    with _Knobs(yf, m), torch.no_grad():
        want = m.forward_u8(u8, (256, 320))
        torch.cuda.synchronize(dev)
        _poisoned(yf, m, dev, u8, 256, 320, call, want)


@pytest.mark.parametrize("size", [(101, 77), (300, 400)], ids=_ID)
def test_forward_bgr_u8_keeps_its_resized_frames_inside_the_workspace(yf, models, dev, size):
    """cvtColor + resize write the net-sized u8 frames at the END of the workspace: the last bytes yf_workspace_bytes counts."""
    m = models["shipped"]
    bgr = torch.from_numpy(np.random.default_rng(size[1]).integers(0, 256, (3,) + size + (3,), dtype=np.uint8)).to(dev)

    def call(e, x, hl, hs, ws, need):
        yf._lib.check(e.lib.yf_forward_bgr_u8(e.handle, x.data_ptr(), 3, size[0], size[1], 15, hl.data_ptr(), hs.data_ptr(), ws.data_ptr(), need,
                                              _stream(dev)))
    with _Knobs(yf, m), torch.no_grad():
        want = m.forward_bgr_u8(bgr, (256, 320))        # (an eager call: the resize tables of this size exist from here on)
        torch.cuda.synchronize(dev)
        _poisoned(yf, m, dev, bgr, 256, 320, call, want)


@pytest.mark.parametrize("precision", rp.PRECISIONS)
def test_two_lanes_keep_to_their_regions(yf, models, golden, dev, precision):
    """chunk 1 on two lanes, three frames of 256 x 320: the per-lane workspace regions and, for f32, the per-lane split-sum scratch."""
    m = models["shipped"]
    x = bo.preprocess(rp.frames_u8(golden, 256, 320, 3)).to(dev)
    with _Knobs(yf, m, precision, chunk=1, lanes=2), torch.no_grad():
        want = m(x)
        e = m.engine(256, 320, 3, dev)
        assert (e.chunk, e.lanes) == (1, 2)
        torch.cuda.synchronize(dev)
        _poisoned(yf, m, dev, x, 256, 320, _forward(yf, dev), want)


@pytest.mark.parametrize("kmax", [16, 1024])
def test_packed_post_process_writes_its_record_block_only(yf, models, golden, dev, kmax):
    """yf_decode_nms_packed on dense logits, heads and record block in the arena: K_max 16 takes the per-frame form (and overflows: the
    first 16 are stored), 1024 the per-class form.  Records are compared up to each frame's count; what lies behind is not specified."""
    m = models["shipped"]
    g = golden("golden_dense_256")
    io = yf.io_params_for(256)
    hl, hs = torch.from_numpy(g["head_large"]).to(dev), torch.from_numpy(g["head_small"]).to(dev)
    N = hl.shape[0]
    post = yf.YOLO_post_process(io["conf_thre"], io["nms_thre"], io["num_anchors"], io["num_cls"], io["anchors"], io["input_shape"]).bind(m)
    # yf_engine.hip post_split_on, auto mode: one workgroup per frame AND class when the caller reserves K_max >= 256, the model has <= 8
    # classes and one workgroup per frame would leave half of the CUs idle
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    per_class = m.post_split == 0 and kmax >= 256 and io["num_cls"] <= 8 and 2 * N <= n_cu
    assert per_class == (kmax == 1024), (kmax, N, n_cu, m.post_split)
    with _Knobs(yf, m):
        e = m.engine(256, 320, N, dev)
        assert e.post_split == 0

        def trimmed(rec):
            v = post.record_views(rec, kmax)
            counts = v["counts"].cpu()
            out = {"counts": v["counts"]}
            for k in ("boxes", "scores", "cls", "src"):
                out[k] = torch.cat([v[k][f, :max(0, min(int(c), kmax))].reshape(-1) for f, c in enumerate(counts)])
            return out
        want = trimmed(post.detect_raw((hl, hs), kmax=kmax, packed=True)["records"])
        torch.cuda.synchronize(dev)
        assert int(want["counts"].max()) > 16 and want["boxes"].numel() > 0
        assert torch.isfinite(want["scores"]).all()

        def run(a):
            l, s = a.put(hl, "head_large"), a.put(hs, "head_small")
            rec = a.empty((N, 1 + 8 * kmax), torch.int32, "records")
            yf._lib.check(e.lib.yf_decode_nms_packed(e.handle, l.data_ptr(), s.data_ptr(), N, float(io["conf_thre"]), float(io["nms_thre"]),
                                                     post._anc, 0, 0, kmax, rec.data_ptr(), _stream(dev)))
            torch.cuda.synchronize(dev)
            return dict(trimmed(rec), head_large=l, head_small=s)
        ar.run_fills(dev, ar.room([hl.numel() * 4, hs.numel() * 4, N * (1 + 8 * kmax) * 4]), run, dict(want, head_large=hl, head_small=hs))


@pytest.mark.parametrize("size", [(96, 160), (256, 320), (256, 352)], ids=_ID)
@pytest.mark.parametrize("precision", rp.PRECISIONS)
def test_a_nan_frame_stays_alone(yf, models, golden, dev, precision, size):
    """Frames 0 and 2 all NaN: frame 1's heads are bitwise those of the same frame run alone (default mode: a frame's bits do not depend
    on the batch it travels in).  A load that crosses a frame boundary and is masked by a product would carry the NaN over."""
    H, W = size
    m = models["shipped"]
    x = bo.preprocess(rp.frames_u8(golden, H, W, 3)).to(dev)
    x[0] = float("nan")
    x[2] = float("nan")
    with _Knobs(yf, m, precision), torch.no_grad():
        alone = m(x[1:2].contiguous())
        hl, hs = m(x)
        torch.cuda.synchronize(dev)
    assert torch.isfinite(alone[0]).all() and torch.isfinite(alone[1]).all()
    assert torch.equal(hl[1:2], alone[0]) and torch.equal(hs[1:2], alone[1]), (
        int((~torch.isfinite(hl[1])).sum()), int((~torch.isfinite(hs[1])).sum()))
