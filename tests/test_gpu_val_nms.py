"""The validation-time decode and NMS (`val_decode_kernel`, `val_nms_kernel` behind yf_val_decode_head / yf_val_nms_ex,
`validation.YOLOLossV3(...)(x)`, `validation.non_max_suppression`) beyond what the trained-network goldens reach: the synthetic cases of
tests/val_cases.py (tests/test_cpu_val_cases.py shows, with the oracle alone, that each case does what it names).

  * NMS: `oracle/val_oracle.py::non_max_suppression` on the same tensor, frame by frame: None against None, else torch.equal -- values,
    order and the +-inf corners of saturated boxes.  No tolerance: after the decode there is only fp32 add / mul / div / compare.
  * decode: the oracle's formulae in float64 (val_cases.decode_f64), in fp32 ulps; the bound is torch's own fp32 decode's worst error on
    the same inputs plus 2 ulp.
  * 512x640 end to end on the shipped checkpoint (M = 4800: the first size whose sort pad needs more than 48 KiB of LDS)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import val_cases as vc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WDIR = os.path.join(ROOT, "yolo-fastest-and-embedded-deployment_amd", "assets", "weights")
WEIGHTS = {256: os.path.join(WDIR, "yolo_fastest_256x320_epoch28.pth"),
           512: os.path.join(WDIR, "yolo_fastest_512x640_epoch27.pth")}


@pytest.fixture(scope="module")
def yf():
    import yolo_fastest_amd
    return yolo_fastest_amd


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


_MODELS = {}


def _model(yf, dev, res):
    if res not in _MODELS:
        io = yf.io_params_for(res)
        m = yf.YoloFastest(io).to(dev).eval()
        m.load_state_dict(torch.load(WEIGHTS[res], map_location=dev))
        _MODELS[res] = (m, io)
    return _MODELS[res]


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _count(d):
    return 0 if d is None else d.shape[0]


def _assert_same(got, want, what):
    assert len(got) == len(want)
    for f, (g, w) in enumerate(zip(got, want)):
        assert (g is None) == (w is None), (what, f, _count(g), _count(w))
        if w is not None:
            g = g.cpu()
            assert g.shape == w.shape, (what, f, tuple(g.shape), tuple(w.shape))
            if not torch.equal(g, w):
                bad = (g != w).any(1).nonzero().flatten()
                raise AssertionError("%s frame %d: %d of %d rows differ, first at %d: %s != %s"
                                     % (what, f, len(bad), len(w), int(bad[0]), g[bad[0]].tolist(), w[bad[0]].tolist()))


@pytest.mark.parametrize("group", [g for g in vc.GROUPS if g != "overflow"])
def test_nms_matches_the_oracle_bit_for_bit(yf, dev, group):
    """every case of the group through validation.non_max_suppression on the device against the oracle on the same tensor"""
    from yolo_fastest_amd import validation as val
    m, _ = _model(yf, dev, 256)
    for c in vc.cases(group):
        got = val.non_max_suppression(c.pred.to(dev), c.C, conf_thres=c.conf_thres, nms_thres=c.nms_thres, model=m)
        _assert_same(got, vc.reference(c), c.name)


def test_nms_of_one_frame_does_not_depend_on_its_batch(yf, dev):
    """the ragged batch (K = 900, 0, 1, 0, 1200) frame by frame: one workgroup per frame, nothing carried from one to the next"""
    from yolo_fastest_amd import validation as val
    m, _ = _model(yf, dev, 256)
    (c,) = vc.cases("ragged")
    ref = vc.reference(c)
    for f in (4, 1, 0, 2):
        got = val.non_max_suppression(c.pred[f:f + 1].to(dev), c.C, conf_thres=c.conf_thres, nms_thres=c.nms_thres, model=m)
        _assert_same(got, ref[f:f + 1], "ragged alone %d" % f)


def _nms_abi(m, dev, pred, C, conf, nms, kmax, M=None):
    e = m.engine_on(dev)
    bs = pred.shape[0]
    det = torch.full((bs, kmax, 7), -7.0, dtype=torch.float32, device=dev)
    cnt = torch.full((bs,), -7, dtype=torch.int32, device=dev)
    rc = e.lib.yf_val_nms_ex(e.handle, pred.data_ptr(), bs, pred.shape[1] if M is None else M, C, conf, nms, kmax, det.data_ptr(),
                             cnt.data_ptr(), _stream(dev))
    torch.cuda.synchronize(dev)
    return rc, det.cpu(), cnt.cpu().tolist(), e.lib.yf_last_error_string().decode()


def test_more_survivors_than_kmax(yf, dev):
    """kmax = 64 and a frame with more survivors: the wrapper raises OverflowError; at the C ABI counts[f] is the TRUE count, the first
    64 rows are the oracle's first 64, and nothing is written past them."""
    from yolo_fastest_amd import validation as val
    m, _ = _model(yf, dev, 256)
    (c,) = vc.cases("overflow")
    ref = vc.reference(c)
    pred = c.pred.to(dev)
    with pytest.raises(OverflowError):
        val.non_max_suppression(pred, c.C, conf_thres=c.conf_thres, nms_thres=c.nms_thres, kmax=vc.OVERFLOW_KMAX, model=m)
    rc, det, cnt, _ = _nms_abi(m, dev, pred, c.C, c.conf_thres, c.nms_thres, vc.OVERFLOW_KMAX)
    assert rc == 0 and cnt == [_count(r) for r in ref] and cnt[1] > vc.OVERFLOW_KMAX
    for f, r in enumerate(ref):
        n = min(cnt[f], vc.OVERFLOW_KMAX)
        if n:
            assert torch.equal(det[f, :n], r[:n]), f
        assert bool((det[f, n:] == -7.0).all())
    _assert_same(val.non_max_suppression(pred, c.C, conf_thres=c.conf_thres, nms_thres=c.nms_thres, model=m), ref, "overflow, kmax = M")


def test_refusals_and_the_largest_class_count(yf, dev):
    """the fields of the sort key: 13 bits of row (M <= 8191), the class above bit 45 (num_classes < 2^18).  Outside them, and for
    num_classes = 0, YF_E_INVALID and no launch; 2^18 - 1 classes still sort and argmax right."""
    from yolo_fastest_amd import _lib, validation as val
    m, _ = _model(yf, dev, 256)
    pred = torch.zeros((1, 8192, 8), dtype=torch.float32, device=dev)
    rc, det, cnt, msg = _nms_abi(m, dev, pred, 3, 0.5, 0.2, 16)
    assert rc == _lib.YF_E_INVALID and "8191" in msg and cnt == [-7] and bool((det == -7.0).all())
    rc, _, cnt, _ = _nms_abi(m, dev, pred, 3, 0.5, 0.2, 16, M=8191)
    assert rc == 0 and cnt == [0]
    rc, _, cnt, _ = _nms_abi(m, dev, pred, 0, 0.5, 0.2, 16, M=64)
    assert rc == _lib.YF_E_INVALID and cnt == [-7]
    rc, _, cnt, msg = _nms_abi(m, dev, pred, 1 << 18, 0.5, 0.2, 16, M=1)
    assert rc == _lib.YF_E_INVALID and "classes" in msg and cnt == [-7]
    with pytest.raises(_lib.YFError):
        val.non_max_suppression(pred, 3, model=m)
    C = (1 << 18) - 1
    p = torch.zeros((1, 4, 5 + C), dtype=torch.float32)
    p[0, :, :4] = torch.tensor([[100.0, 100, 50, 50], [300, 300, 40, 40], [104, 100, 50, 50], [500, 100, 30, 30]])
    p[0, :, 4] = torch.tensor([0.6, 0.9, 0.8, 0.7])
    p[0, 0, 5 + C - 1] = p[0, 2, 5 + C - 1] = 0.5         # rows 0 and 2: the last class, overlapping
    p[0, 1, 5] = 0.5                                       # row 1: class 0
    p[0, 3, 5 + (1 << 17)] = 0.5
    from oracle import val_oracle as vo
    want = vo.non_max_suppression(p, C, 0.5, 0.2)
    assert want[0][:, 6].tolist() == [0.0, float(1 << 17), float(C - 1)]
    _assert_same(val.non_max_suppression(p.to(dev), C, conf_thres=0.5, nms_thres=0.2, model=m), want, "2^18 - 1 classes")


# ---- decode ----------------------------------------------------------------------------------------------------------------------

def _decode_abi(m, dev, H, W, head, anchors, out, m_off):
    e = m.engine(H, W, head.shape[0], dev)
    anc = (ctypes.c_double * (2 * len(anchors)))(*[float(v) for a in anchors for v in a[:2]])
    rc = e.lib.yf_val_decode_head(e.handle, head.data_ptr(), head.shape[0], head.shape[2], head.shape[3], anc, out.shape[1], m_off,
                                  out.data_ptr(), _stream(dev))
    torch.cuda.synchronize(dev)
    return rc


# (model, H, W, fh, fw, anchor group): the grids of both shipped sizes, a 32x32 input (2x2 and 1x1 cells), and -- C ABI only -- a 3x5 grid on
# the 32x32 engine, whose strides 32/3 and 32/5 are not fp32 numbers
DECODE_GRIDS = ((256, 256, 320, 16, 20, 0), (256, 256, 320, 8, 10, 1), (512, 512, 640, 32, 40, 0), (512, 512, 640, 16, 20, 1),
                (256, 32, 32, 2, 2, 0), (256, 32, 32, 1, 1, 1), (256, 32, 32, 3, 5, 1))
# The bound of test_decode_against_float64: torch's own worst fp32 error on the same inputs + DECODE_EXTRA_ULP, per group of outputs.
# Measured on an MI355X (torch-CPU fp32 / val_decode_kernel, worst fp32 ulps from float64):
#   N(0, 4) logits 1.93 / 1.91;  planted logits 849.52 / 849.52 (from the tiny results: exp(-100) is a 5-bit subnormal before the
#   anchor multiplies it)
DECODE_EXTRA_ULP = 2.0      # HIP's expf is a 1-ulp function; the sigmoid composes it with one add and one divide


def test_decode_against_float64(yf, dev, capsys):
    """Every output of val_decode_kernel against the oracle's formulae in float64 (on the fp32-rounded strides and anchors the C ABI
    computes), in fp32 ulps of the float64 value.  Bound: the worst error of torch's own fp32 decode (val_oracle.decode_head) on the same
    inputs + 2 ulp, separately for the random logits and for the planted ones: sigmoid(-100) is a subnormal that both fp32 evaluations
    flush to 0 through exp(100) = inf, and exp(-100) is a subnormal of 5 significant bits before it is multiplied by the anchor --
    hundreds of subnormal ulps for any fp32 evaluation of these formulae, which must not widen the bound of the random logits.  Where float64 rounds to +inf in fp32, or is exactly 0 or 1, the kernel gives exactly that."""
    from oracle import val_oracle as vo
    from yolo_fastest_amd import validation as val
    worst = {"bulk": [0.0, 0.0], "planted": [0.0, 0.0]}          # [torch, kernel]
    for i, (res, H, W, fh, fw, grp) in enumerate(DECODE_GRIDS):
        m, io = _model(yf, dev, res)
        anchors = io["anchors"][grp]
        x, planted = vc.decode_head(100 + i, 3, 3, 3, fh, fw)
        xd = torch.from_numpy(x).to(dev)
        if (fh * 16, fw * 16) == (H, W) or (fh * 32, fw * 32) == (H, W):
            got = val.YOLOLossV3(anchors, 3, [H, W, 1], dev, model=m)(xd)
        else:
            got = torch.empty((3, 3 * fh * fw, 8), dtype=torch.float32, device=dev)
            assert _decode_abi(m, dev, H, W, xd, anchors, got, 0) == 0
        got = got.cpu().numpy()
        ref32 = vo.decode_head(torch.from_numpy(x), anchors, 3, [H, W]).numpy()
        want = vc.decode_f64(x, anchors, 3, H, W)
        assert got.shape == want.shape == ref32.shape
        with np.errstate(over="ignore"):
            w32 = want.astype(np.float32)
        assert np.array_equal(np.isinf(w32), np.isinf(got)) and np.array_equal(got[np.isinf(w32)], w32[np.isinf(w32)]), (fh, fw)
        exact = (want == 0.0) | (want == 1.0)
        assert np.array_equal(got[exact], w32[exact]), (fh, fw)
        assert not np.isnan(got).any()
        pl = planted.reshape(3, 3, 8, fh, fw).transpose(0, 1, 3, 4, 2).reshape(want.shape)
        e_t, e_k = vc.ulp_error(ref32, want), vc.ulp_error(got, want)
        for name, mask in (("bulk", ~pl), ("planted", pl)):
            if mask.any() and not np.isnan(e_k[mask]).all():
                worst[name][0] = max(worst[name][0], float(np.nanmax(e_t[mask])))
                worst[name][1] = max(worst[name][1], float(np.nanmax(e_k[mask])))
    with capsys.disabled():
        for name, (t, k) in worst.items():
            print(f"\n[val decode vs float64, {name} logits] worst error: torch fp32 {t:.2f} ulp, val_decode_kernel {k:.2f} ulp")
    for name, (t, k) in worst.items():
        assert k <= t + DECODE_EXTRA_ULP, (name, k, t)



def test_decode_into_one_tensor_with_m_off(yf, dev):
    """yf_val_decode_head's concatenating form: two calls (m_off = 0 and A fh fw) into one [N, M_total, 5 + C] tensor = torch.cat of the two
    single-head calls bit for bit; with M_total 7 rows larger than needed the spare rows are not touched."""
    m, io = _model(yf, dev, 256)
    heads = [torch.from_numpy(vc.decode_head(200 + i, 3, 3, 3, fh, fw)[0]).to(dev) for i, (fh, fw) in enumerate(((16, 20), (8, 10)))]
    M0, M1 = 3 * 16 * 20, 3 * 8 * 10
    single = []
    for h, grp, M in ((heads[0], 0, M0), (heads[1], 1, M1)):
        out = torch.empty((3, M, 8), dtype=torch.float32, device=dev)
        assert _decode_abi(m, dev, 256, 320, h, io["anchors"][grp], out, 0) == 0
        single.append(out)
    want = torch.cat(single, 1).cpu()
    pattern = 0x7FC12345                                      # a NaN with a payload
    for spare in (0, 7):
        both = torch.full((3, M0 + M1 + spare, 8), pattern, dtype=torch.int32, device=dev).view(torch.float32)
        assert _decode_abi(m, dev, 256, 320, heads[0], io["anchors"][0], both, 0) == 0
        assert _decode_abi(m, dev, 256, 320, heads[1], io["anchors"][1], both, M0) == 0
        bits = both.cpu().view(torch.int32)
        assert torch.equal(bits[:, :M0 + M1], want.view(torch.int32))
        assert bool((bits[:, M0 + M1:] == pattern).all())
    from yolo_fastest_amd import _lib
    both = torch.zeros((3, M0 + M1, 8), dtype=torch.float32, device=dev)
    assert _decode_abi(m, dev, 256, 320, heads[1], io["anchors"][1], both, M0 + 1) == _lib.YF_E_INVALID      # one row past the end
    assert _decode_abi(m, dev, 256, 320, heads[1], io["anchors"][1], both, -1) == _lib.YF_E_INVALID
    assert not bool(both.any())


# ---- 512x640 end to end -----------------------------------------------------------------------------------------------------------

def test_validation_chain_at_512x640(yf, dev, golden, capsys):
    """The shipped 512x640 checkpoint on the first 4 bundled frames: model, the two YOLOLossV3 decodes and non_max_suppression on the device
    (M = 4800 rows: 8192-row sort pad, 79 KiB of dynamic LDS) against backbone_oracle.forward, val_oracle.decode and
    val_oracle.non_max_suppression on the CPU: the same number of survivors and the same classes in every frame.

    Values: 2e-6 relative + 2e-5 absolute is the tolerance of the DECODE given identical logits (test_validation_path_decode_and_nms).
    Here the logits are two fp32 evaluations of the network; the oracle's own fp32 logits are E away from the graph in float64 on these
    frames (E is printed; 5.7e-4 over the 20 frames of this size, tests/test_gpu_parity.py header), the device's at most 3 E
    (_check_heads), so the two are up to 4 E apart.  A logit error d moves w, h by d w, d h and cx, cy by at most stride d / 4, hence a
    corner by at most d (8 + max(w, h) / 2) and a score by d / 4: those, with d = 4 E, are added to the decode tolerance.

    Then the saturated variant: + 90 on the w logit of frame 0's 5 most confident cells (exp overflows to +inf).  NMS on the device's own
    decode must equal the oracle's NMS on that same tensor bit for bit, and the device's decode of those heads must have its infinities
    exactly where the oracle's decode of the same heads has them (finite values: the decode tolerance)."""
    from oracle import backbone_oracle as bo
    from oracle import val_oracle as vo
    from yolo_fastest_amd import validation as val
    m, io = _model(yf, dev, 512)
    u8 = golden("golden_512")["input_u8"][:4]
    assert u8.shape == (4, 512, 640)
    losses = [val.YOLOLossV3(io["anchors"][i], 3, io["input_shape"], dev, model=m) for i in range(2)]
    with torch.no_grad():
        heads = m(bo.preprocess(u8).to(dev))
    dec = torch.cat([losses[i](heads[i]) for i in range(2)], 1)
    assert dec.shape == (4, 4800, 8)
    got = val.non_max_suppression(dec, 3, conf_thres=0.5, nms_thres=0.2, model=m)
    sd = bo.load_state_dict(WEIGHTS[512])
    o32 = bo.forward(sd, bo.preprocess(u8))
    o64 = bo.forward({k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}, bo.preprocess(u8).double())
    E = max(float((a.double() - b).abs().max()) for a, b in zip(o32, o64))
    with capsys.disabled():
        print(f"\n[512x640, 4 frames] oracle fp32 logits vs float64: E = {E:.3e}; device vs float64: "
              f"{max(float((a.cpu().double() - b).abs().max()) for a, b in zip(heads, o64)):.3e}")
    want = vo.non_max_suppression(vo.decode(list(o32), io["anchors"], 3, io["input_shape"]), 3, 0.5, 0.2)
    assert sum(_count(w) for w in want) >= 4
    d = 4.0 * E
    for f, (g, w) in enumerate(zip(got, want)):
        assert _count(g) == _count(w), (f, _count(g), _count(w))
        if w is None:
            continue
        g = g.cpu()
        assert torch.equal(g[:, 6], w[:, 6]), f
        side = torch.maximum(w[:, 2] - w[:, 0], w[:, 3] - w[:, 1])
        tol = torch.empty_like(w[:, :6])
        tol[:, :4] = (2e-5 + 2e-6 * w[:, :4].abs()) + d * (8.0 + side[:, None] / 2)
        tol[:, 4:6] = (2e-5 + 2e-6 * w[:, 4:6].abs()) + d / 4
        assert bool(((g[:, :6] - w[:, :6]).abs() <= tol).all()), (f, (g[:, :6] - w[:, :6]).abs().max(0).values.tolist(), tol.max(0).values.tolist())
    # the device NMS on the device's own decode tensor is the oracle's NMS on it, bit for bit (M = 4800, trained logits)
    _assert_same(got, vo.non_max_suppression(dec.cpu(), 3, 0.5, 0.2), "512x640, own decode")

    # saturated: + 90 on the w logit of the 5 most confident cells of frame 0
    f = 0
    top = torch.topk(dec[f, :, 4], 5).indices.tolist()
    sat = [h.clone() for h in heads]
    for r in top:
        hd, r = (0, r) if r < 3 * 32 * 40 else (1, r - 3 * 32 * 40)
        fh, fw = sat[hd].shape[2:]
        a, i, j = r // (fh * fw), (r % (fh * fw)) // fw, r % fw
        sat[hd][f, a * 8 + 2, i, j] += 90.0
    dec_s = torch.cat([losses[i](sat[i]) for i in range(2)], 1)
    ref_s = vo.decode([h.cpu() for h in sat], io["anchors"], 3, io["input_shape"])
    assert torch.isinf(ref_s[f, top, 2]).all() and int(torch.isinf(ref_s).sum()) == 5
    ds = dec_s.cpu()
    assert torch.equal(torch.isinf(ds), torch.isinf(ref_s)) and torch.equal(ds[torch.isinf(ref_s)], ref_s[torch.isinf(ref_s)])
    fin = ~torch.isinf(ref_s)
    assert bool(((ds[fin] - ref_s[fin]).abs() <= 2e-6 * max(1.0, float(ref_s[fin].abs().max()))).all())
    got_s = val.non_max_suppression(dec_s, 3, conf_thres=0.5, nms_thres=0.2, model=m)
    want_s = vo.non_max_suppression(ds, 3, 0.5, 0.2)
    assert bool(torch.isinf(want_s[f][:, :4]).any())                       # an infinite box is kept and meets the rest of its class
    _assert_same(got_s, want_s, "512x640 saturated, own decode")
    # ... and through the oracle's decode of the device's own heads: the same survivors and classes
    want_o = vo.non_max_suppression(ref_s, 3, 0.5, 0.2)
    for g, w in zip(got_s, want_o):
        assert _count(g) == _count(w) and (w is None or (torch.equal(g.cpu()[:, 6], w[:, 6])
                                                         and torch.equal(torch.isinf(g.cpu()), torch.isinf(w))))
        if w is not None:
            gg, fin = g.cpu(), ~torch.isinf(w)
            assert torch.allclose(gg[fin], w[fin], rtol=2e-6, atol=2e-5)
