"""The trainer's backward (yf_trainer_forward / yf_trainer_backward, csrc/yf_train_engine.hip) against a float64 replay on the device's
own tape (oracle/train_replay.py; the CPU side of the method is tests/test_cpu_train_replay.py).

The trainer does not run the operators as the operator tests call them: BatchNorm's forward sums come out of the conv's epilogue
(TStatPart), its backward sums out of the depthwise data-gradient kernel of the layer above (TBnRed), a pointwise layer's two
gradients are one launch (tpw_bwd_dual_kernel), the skip gradient and the residual are fused, the split weight-gradient sums are
deferred to one launch.  Which layer takes which form depends on N, H, W; `forms()` below restates the launchers' conditions
(csrc/yf_train_kernels.hip, yf_train_dw_kernels.h, yf_train_engine.hip) and every configuration prints its table and asserts the
forms it is there for.  Configurations = the smallest that switch each form:

  A  N=3, 64x96 (two seeds)   no partial sums anywhere, every BatchNorm one launch; dual kernel on at strides 2..8, off at 16 / 32
                              (N*HW < 256), where the skip gradient goes through launch_tpw_gemm's addend
  D  N=9, 96x160              N*48*80 = 34560 > 32768: stat parts (pointwise Cout <= 32, depthwise rows kernel with 240 row groups in one
                              256-thread workgroup) and TBnRed at stride 2 only; 6x10 and 3x5 maps: plane kernels (W % 4 != 0), the
                              H % 4 != 0 fallbacks, and at 3x5 HW % 4 != 0: no dual kernel, scalar BatchNorm
  B  N=40, 256x256            parts and TBnRed at strides 2, 4 and 8 (the rows kernel at its edge (H/4)*(W/4) = 64 at stride 8), the
                              split 3x3 stride-2 weight-gradient kernels, the many-small-planes depthwise form at 16x16,
                              one-launch BatchNorm at strides 16 (10240 <= 32768 with HW % 4 == 0) and 32, dual kernel everywhere
  C  N=132, 256x256           replayed from res4_1.conv1 on (strides 16 and 32): N*16*16 = 33792 > 32768, the deep stage's regime at
                              the benchmark batch -- pointwise stat parts where Cout <= 32 (the four res4_x.conv3; the 136 / 232 -> 96
                              channel layers have mt = 3 channel tiles per wave and take none), two-launch BatchNorm at stride 16
                              with and without parts, one-launch at stride 32

Acceptance is train_replay.compare(): per tensor e = max|g - g64| / max|g64|; median and 90th percentile of the device at most 2x
those of the CPU fp32 twin (the same replay in float32), every tensor within 8 x max(its twin's error, the twin's median), the 23
BatchNorm biases whose gradient is zero in exact arithmetic within 8x the twin's noise.  Per-unit forward errors (the tape's z against
conv(x_tape), y against act(bn(z_tape)), float64) at the operator tests' 3e-6.

MEASURED (MI355X; per tensor relative to its largest element; the test prints them with the five tensors closest to their bound):
  config   device median / p90 / max      fp32 twin median / p90 / max     worst tensor vs its bound's base   zero set device / twin   forward conv / BatchNorm
  A seed 1 8.4e-7 / 1.4e-6 / 3.1e-6       8.4e-7 / 1.5e-6 / 3.7e-6         2.5x (res5_1.conv1.1.weight)       1.3e-3 / 1.7e-2          5.7e-7 / 1.3e-7
  A seed 2 6.5e-7 / 1.2e-6 / 2.5e-6       7.3e-7 / 1.3e-6 / 4.6e-6         2.2x (res4_3.conv1.1.bias)         1.0e-3 / 3.2e-3          6.2e-7 / 1.3e-7
  D        7.2e-7 / 1.3e-6 / 3.0e-6       7.6e-7 / 1.5e-6 / 1.1e-5         1.9x (conv3_1.1.weight)            2.4e-3 / 2.3e-2          4.2e-7 / 1.3e-7
  B        7.9e-7 / 1.3e-6 / 3.7e-6       9.9e-7 / 3.8e-6 / 3.1e-5         1.8x (conv3_1.1.weight)            2.7e-2 / 4.9e-1          5.3e-7 / 1.3e-7
  C        6.3e-7 / 9.9e-7 / 2.1e-6       8.3e-7 / 3.2e-6 / 1.1e-5         1.3x (res4_3.conv1.0.weight)       9.0e-4 / 2.9e-3          4.5e-7 / 1.4e-7
Every configuration is inside the rule as stated (2x / 8x / 8x); none is pinned separately.  The device is at or below the twin
everywhere: its BatchNorm sums are in double, torch's fp32 ones are not, which shows at the long sums of B and C.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import backbone_oracle as bo  # noqa: E402
from oracle import train_replay as tr  # noqa: E402


@pytest.fixture(scope="module")
def yf():
    import yolo_fastest_amd
    return yolo_fastest_amd


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops(yf, dev):
    from yolo_fastest_amd import training
    return training._Ops(dev)


def _g(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def _close(got, want, rel, what):
    got = got.cpu().numpy().astype(np.float64)
    want = want.detach().numpy().astype(np.float64)
    assert got.shape == want.shape, what
    err = np.abs(got - want).max()
    assert err <= rel * max(np.abs(want).max(), 1e-30), (what, err, np.abs(want).max())


# ---- which layer takes which form: the launchers' conditions, restated ----
PARTS_MIN = 4096 * 8           # launch_tconv_fwd / launch_tconv_bwd_data: partial sums only above this many samples per channel
PART_ROOM = (32 << 20) - (1 << 20)


def _mt(M, Q):
    """launch_tpw_gemm / launch_tpw_bwd_dual: channel tiles per wave."""
    tiles = (M + 15) // 16
    mgroups = (tiles + 3) // 4
    mt = -(-tiles // mgroups)
    while mt > 1 and (Q + 63) // 64 * mgroups < 512:
        mt = (mt + 1) // 2
        mgroups = -(-tiles // mt)
    return mt


def _rows(H, W):
    return H % 4 == 0 and (H // 4) * (W // 4) >= 64


def _rows_groups(H, W):
    """launch_tdw_conv: workgroups per plane of the rows kernel."""
    count = (H // 4) * (W // 4)
    bs, waste = 256, -(-count // 256) * 256 - count
    for b in (192, 128, 64):
        if -(-count // b) * b - count < waste:
            bs, waste = b, -(-count // b) * b - count
    return -(-count // bs), bs


def _bn_form(P, HW, parts):
    if HW % 4 == 0 and P <= PARTS_MIN:
        return "one launch (float4)"
    if P <= 8192:
        return "one launch (scalar)"
    flat = HW % 4 == 0 and HW % 1024 != 0
    return "two launches%s, %s" % (" from parts" if parts else "", "flat float4" if flat else "float4" if HW % 4 == 0 and HW >= 1024 else "scalar")


def forms(N, H, W):
    """{unit: {map, fwd_parts, bn_fwd, bn_bwd, wgrad, dgrad, skip}} for a batch of N frames of HxW."""
    geo, out, prev = {}, {}, None
    for name, kind, cin, cout, k, s, relu in bo.LAYERS:
        src = {"deconv5_1": "conv5_2", "conv4_1_1": "conv4_2"}.get(name, prev)
        Hin, Win = geo[src][:2] if src else (H, W)
        Ho, Wo = (2 * Hin, 2 * Win) if kind == "dc" else ((Hin + 2 * ((k - 1) // 2) - k) // s + 1, (Win + 2 * ((k - 1) // 2) - k) // s + 1)
        geo[name] = (Ho, Wo, Hin, Win, src)
        prev = name
    for name, kind, cin, cout, k, s, relu in bo.LAYERS:
        Ho, Wo, Hin, Win, src = geo[name]
        P, HW, Q = N * Ho * Wo, Ho * Wo, N * Hin * Win
        pw = kind == "c" and k == 1
        f = dict(map="%dx%d" % (Ho, Wo), fwd_parts="", skip="")
        if kind != "dc" and P > PARTS_MIN:
            if pw and _mt(cout, P) <= 2 and HW % 4 == 0 and cin % 4 == 0 and (P + 255) // 256 * 4 * cout * 8 <= PART_ROOM:
                f["fwd_parts"] = "pointwise epilogue"
            if kind == "dw" and s == 1 and not (Win % 4 != 0 and Win <= 16) and Wo % 4 == 0 and _rows(Hin, Win):
                f["fwd_parts"] = "rows kernel, %d workgroup(s) of %d per plane" % _rows_groups(Hin, Win)
        f["bn_fwd"] = _bn_form(P, HW, bool(f["fwd_parts"])) + (" + residual" if name.endswith(".conv3") else "")
        need_dx = name != "conv0"
        block_in = name.endswith(".conv1")
        dual = pw and need_dx and HW % 4 == 0 and cout % 4 == 0 and 256 <= Q <= 2000000
        if dual:
            f["wgrad"] = f["dgrad"] = "dual kernel"
        elif kind == "dc":
            f["wgrad"], f["dgrad"] = ("mfma split" if (Hin * Win) % 4 == 0 else "atomics"), ("mfma" if Q >= 256 else "scalar")
        elif kind == "c":
            G = N * Ho * (Wo // 4)
            if k == 3 and s == 2 and Hin % 2 == 0 and Win % 8 == 0 and cin == 1 and cout <= 8 and G >= 4096:
                f["wgrad"] = "3x3 stride 2, Cin 1, split"
            elif k == 3 and s == 2 and Hin % 2 == 0 and Win % 8 == 0 and cin % 4 == 0 and cin <= 32 and cout <= 32 and G >= 2048:
                f["wgrad"] = "3x3 stride 2 mfma, split"
            else:
                f["wgrad"] = ("mfma split" + (", 4 waves per slice" if P >= 65536 else "")) if HW % 4 == 0 and (k == 3 or s == 1) else "atomics"
            f["dgrad"] = "tpw_gemm" if pw else "-" if not need_dx else "3x3 stride 2"
        else:
            f["wgrad"] = ("rows" if s == 1 and Win % 4 == 0 and Hin % 4 == 0 and N * (Hin // 4) * (Win // 4) >= 2048 else
                          "plane" if s == 1 and Win % 4 != 0 and Win <= 16 else "other")
            f["dgrad"] = ("stride 2" if s == 2 else "plane" if Win % 4 != 0 and Win <= 16 else "rows" if Win % 4 == 0 and _rows(Hin, Win) else
                          "many small planes" if Win % 4 == 0 and Hin % 4 == 0 and N * cin * (Hin // 4) * (Win // 4) >= 16384 else "other")
        if block_in:
            f["skip"] = "addend in the dual kernel" if dual else "addend in tpw_gemm"
        out[name] = f
    for name, kind, cin, cout, k, s, relu in bo.LAYERS:          # TBnRed: the depthwise data-gradient kernel leaves the sums of the layer below
        Ho, Wo, Hin, Win, src = geo[name]
        red = (kind == "dw" and s == 1 and src not in (None, "conv4_2", "conv5_2") and out[name]["dgrad"] == "rows" and N * Hin * Win > PARTS_MIN
               and N * _rows_groups(Hin, Win)[0] * cin * 8 <= PART_ROOM)
        if red:
            out[src]["_red"] = True
    for name, kind, cin, cout, k, s, relu in bo.LAYERS:
        Ho, Wo = geo[name][:2]
        out[name]["bn_bwd"] = _bn_form(N * Ho * Wo, Ho * Wo, out[name].pop("_red", False)).replace("from parts", "from TBnRed parts")
    return out


def _table(fm, names):
    groups = {}
    for n in names:
        f = fm[n]
        key = (f["map"], bo._BY_NAME[n][1] + str(bo._BY_NAME[n][4]), f["fwd_parts"], f["bn_fwd"], f["bn_bwd"], f["wgrad"], f["dgrad"], f["skip"])
        groups.setdefault(key, []).append(n)
    rows = []
    for (mp, kd, fp, bf, bb, wg, dg, sk), ns in groups.items():
        rows.append("  %-8s %-4s x%-2d stat parts: %-44s bn fwd: %-42s bn bwd: %-44s wgrad: %-28s dgrad: %-18s %s | %s"
                    % (mp, kd, len(ns), fp or "-", bf, bb, wg, dg, sk, " ".join(ns)))
    return "\n".join(rows)


#          N, H, W, seed, first_unit, {unit: {key: substring}} the forms the configuration is there for
CONFIGS = {
    "A-seed1": (3, 64, 96, 1, None, {"res1_1.conv3": dict(fwd_parts="", bn_fwd="one launch (float4) + residual", bn_bwd="one launch"),
                                     "conv1_2": dict(fwd_parts="", bn_bwd="one launch"), "res3_3.conv1": dict(skip="dual"),
                                     "res4_1.conv1": dict(skip="tpw_gemm", wgrad="mfma split"), "res5_1.conv1": dict(skip="tpw_gemm")}),
    "A-seed2": (3, 64, 96, 2, None, {}),
    "D": (9, 96, 160, 1, None, {"conv1_2": dict(fwd_parts="pointwise", bn_fwd="from parts", bn_bwd="TBnRed"),
                                "conv1_3": dict(fwd_parts="1 workgroup(s) of 256", dgrad="rows"), "res1_1.conv1": dict(bn_bwd="TBnRed", skip="dual"),
                                "res1_1.conv3": dict(fwd_parts="pointwise", bn_fwd="from parts, flat float4 + residual"),
                                "res2_1.conv2": dict(fwd_parts="", dgrad="many small planes", bn_fwd="one launch"), "res4_1.conv2": dict(dgrad="plane", wgrad="plane"),
                                "conv4_1_2": dict(dgrad="plane"), "res5_1.conv2": dict(dgrad="plane", bn_fwd="one launch (scalar)"),
                                "res5_1.conv1": dict(skip="tpw_gemm", wgrad="atomics"), "conv4_3": dict(wgrad="other")}),
    "B": (40, 256, 256, 1, None, {"conv1_2": dict(fwd_parts="pointwise", bn_bwd="TBnRed"), "res2_1.conv1": dict(bn_bwd="TBnRed", skip="dual"),
                                  "res2_1.conv2": dict(fwd_parts="rows kernel"), "res3_3.conv1": dict(bn_bwd="TBnRed"),
                                  "res3_3.conv2": dict(fwd_parts="1 workgroup(s) of 64", dgrad="rows"), "conv0": dict(wgrad="Cin 1, split"),
                                  "conv1_9": dict(wgrad="stride 2 mfma, split"), "res4_1.conv2": dict(dgrad="many small planes", bn_fwd="one launch (float4)"),
                                  "res5_1.conv2": dict(bn_fwd="one launch (float4)"), "res5_1.conv1": dict(skip="dual"), "res4_1.conv1": dict(skip="dual")}),
    "C": (132, 256, 256, 1, "res4_1.conv1", {"res4_1.conv3": dict(fwd_parts="pointwise", bn_fwd="two launches from parts, flat float4 + residual"),
                                             "res4_1.conv1": dict(fwd_parts="", bn_fwd="two launches, flat float4", bn_bwd="two launches, flat float4"),
                                             "conv4_1_1": dict(fwd_parts="", bn_fwd="two launches"), "deconv5_1": dict(bn_fwd="two launches"),
                                             "res5_1.conv3": dict(bn_fwd="one launch (float4) + residual"), "res4_1.conv2": dict(dgrad="many small planes")}),
}
FWD_TOL = 3e-6        # test_large_map_kernels_match_torch (conv forward), test_batchnorm_train_mode_matches_torch (BatchNorm forward)


def _model(yf, sd0, dev):
    m = yf.YoloFastest(yf.io_params_for(256))
    m.load_state_dict(sd0)
    return m.to(dev).train()


def _inputs(N, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((N, 1, H, W), generator=g) - 0.5, torch.randn((N, 24, H // 16, W // 16), generator=g),
            torch.randn((N, 24, H // 32, W // 32), generator=g))


@pytest.mark.parametrize("config", list(CONFIGS))
def test_trainer_backward_against_the_float64_replay_of_its_own_tape(yf, dev, capsys, config):
    """Default train_impl (the trainer), random weights with non-zero BatchNorm biases, random head gradients.  The tape is the per-block
    path's on a twin model (its heads must be bit-equal to the trainer's: then it IS the trainer's tape); per-unit forward errors and
    all parameter gradients against the float64 replay, judged by train_replay.compare with the CPU fp32 replay as yardstick."""
    from random_weights import random_state_dict
    from yolo_fastest_amd import training
    N, H, W, seed, first, expect = CONFIGS[config]
    fm = forms(N, H, W)
    for unit, want in expect.items():
        for key, sub in want.items():
            assert (sub in fm[unit][key]) if sub else fm[unit][key] == "", (config, unit, key, fm[unit][key])
    sd0 = random_state_dict(seed)
    assert min(float(v.abs().min()) for k, v in sd0.items() if k.endswith(".1.bias")) > 0
    x, g_hl, g_hs = _inputs(N, H, W, seed)
    xd = x.to(dev)
    m = _model(yf, sd0, dev)
    assert getattr(m, "train_impl", "trainer") == "trainer"
    hl, hs = m(xd)
    torch.autograd.backward([hl, hs], [g_hl.to(dev), g_hs.to(dev)])
    g_dev = {n: p.grad.cpu() for n, p in m.named_parameters()}
    hl, hs = hl.detach().clone(), hs.detach().clone()
    del m
    twin = _model(yf, sd0, dev)
    saved = {k: v.clone() for k, v in twin.state_dict().items() if "running_" in k or "num_batches" in k}
    with torch.no_grad():
        hl2, hs2, tape = training.train_forward(twin, xd)
    twin.load_state_dict(saved, strict=False)
    assert torch.equal(hl, hl2) and torch.equal(hs, hs2)
    units = tr.unit_names(first)
    tape = {k: (tuple(t.cpu() if torch.is_tensor(t) else t for t in v) if isinstance(v, tuple) else v.cpu())
            for k, v in tape.items() if k in units or k.startswith("head_")}
    del twin
    torch.cuda.empty_cache()
    g64, fwd = tr.replay(sd0, tape, g_hl, g_hs, torch.float64, first_unit=first)
    g_twin, _ = tr.replay(sd0, tape, g_hl, g_hs, torch.float32, first_unit=first)
    r = tr.compare(g_dev, g64, g_twin)
    wz, wy = max(fwd, key=lambda u: fwd[u][0]), max(fwd, key=lambda u: fwd[u][1])
    with capsys.disabled():
        print("\n[trainer replay %s] N=%d %dx%d%s\n%s" % (config, N, H, W, " from " + first if first else "", r.table()))
        print("  forward: worst conv %.2e (%s), worst BatchNorm %.2e (%s)" % (fwd[wz][0], wz, fwd[wy][1], wy))
        if not config.endswith("seed2"):
            print(_table(fm, units))
    assert list(fwd) == units and len(g64) == 3 * len(units) + 4
    for u in units:
        assert fwd[u][0] <= FWD_TOL and fwd[u][1] <= FWD_TOL, (u, fwd[u], fm[u])
    assert r.ok, "\n".join(r.failures)
    assert len(r.zero) == (23 if first is None else 9) and all(not bo._BY_NAME[k[:-len(".1.bias")]][6] for k in r.zero)   # units without ReLU


def test_trainer_backward_is_the_same_with_and_without_a_flat_gradient_buffer(yf, dev):
    """yf_trainer_backward with the flat parameters()-order gradient buffer training.py passes (the split weight-gradient sums of all
    layers deferred to ONE tsum_multi_kernel launch) and with separately allocated gradient tensors (every layer sums its own slabs):
    the same sums in the same order, so the 256 gradients are bit-identical.  At configuration D."""
    from random_weights import random_state_dict
    from yolo_fastest_amd import _lib, training
    N, H, W, seed = CONFIGS["D"][:4]
    x, g_hl, g_hs = (t.to(dev) for t in _inputs(N, H, W, seed))
    m = _model(yf, random_state_dict(seed), dev)
    params = tuple(m.parameters())
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    keep = []                                   # (every pass with pointers of its own: plain launches, no graph replay in between)

    def backward(grads):
        with torch.no_grad():
            hl, hs, trn, (ws, pp) = training._trainer_forward(m, x, params)
        keep.append((hl, hs, ws))
        gp = (ctypes.c_void_p * len(params))(*[g.data_ptr() for g in grads])
        _lib.check(trn.lib.yf_trainer_backward(trn.handle, x.data_ptr(), g_hl.data_ptr(), g_hs.data_ptr(), N, pp, gp, ws.data_ptr(), ws.numel(), stream))
        torch.cuda.synchronize(dev)
        return trn
    trn = training._trainer(m, H, W, dev)
    lay = trn.layout(params)
    flat = torch.full((lay["total"],), float("nan"), device=dev)
    flat_views = [g.view(s) for g, s in zip(flat.split(lay["sizes"]), lay["shapes"])]
    backward(flat_views)
    apart = [torch.full_like(p, float("nan")) for p in params]
    assert any(b.data_ptr() - apart[0].data_ptr() != 4 * sum(lay["sizes"][:i + 1]) for i, b in enumerate(apart[1:]))     # not the flat layout
    backward(apart)
    for (n, _), a, b in zip(m.named_parameters(), flat_views, apart):
        assert torch.isfinite(a).all() and torch.equal(a, b), (n, float((a - b).abs().max()))


#        deconv? N, Cin, Cout, k, depthwise, H, W     (stride 1; N * H * W > 32768: the conv leaves BatchNorm's partial sums)
UNITS = [(9, 8, 24, 1, 0, 64, 64),      # pointwise: 144 pixel blocks x 4 pairs per channel
         (9, 8, 30, 1, 0, 64, 64),      # Cout no multiple of the 16-row tile
         (9, 8, 24, 1, 0, 60, 68),      # Q % 256 != 0: a ragged last pixel block
         (5, 8, 8, 3, 1, 84, 80),       # depthwise rows kernel: 420 row groups per plane, workgroups of 64, the last one ragged
         (5, 8, 8, 5, 1, 84, 80)]


@pytest.mark.parametrize("geom", UNITS)
@pytest.mark.parametrize("relu", [0, 1])
def test_unit_entry_points_with_stat_parts_match_torch(ops, dev, geom, relu):
    """yf_train_unit_forward / yf_train_unit_backward -- the only C ABI route into TStatPart (tbn_stats_from_parts_kernel) -- against
    conv + train-mode BatchNorm (+ ReLU) of torch in float64: z, y, the saved statistics, the running statistics, dgamma, dbeta, the
    conv-output gradient, dw, dx.  Tolerances: those of test_large_map_kernels_match_torch (conv) and
    test_batchnorm_train_mode_matches_torch (BatchNorm) for the same quantities; mean / invstd like the running statistics."""
    N, Cin, Cout, k, dw, H, W = geom
    fm_parts = (N * H * W > PARTS_MIN) and ((not dw and _mt(Cout, N * H * W) <= 2) or (dw and _rows(H, W)))
    assert fm_parts, geom
    rng = np.random.default_rng(sum(geom) + relu)
    x = (rng.normal(size=(N, Cin, H, W)) * rng.uniform(0.5, 2, (1, Cin, 1, 1)) + rng.normal(size=(1, Cin, 1, 1))).astype(np.float32)
    w = (rng.normal(size=(Cout, 1 if dw else Cin, k, k)) / k).astype(np.float32)
    gamma, beta = rng.normal(1, 0.3, Cout).astype(np.float32), rng.normal(0, 0.5, Cout).astype(np.float32)
    rm, rv = rng.normal(size=Cout).astype(np.float32), rng.uniform(0.5, 2, Cout).astype(np.float32)
    bn = torch.nn.BatchNorm2d(Cout).double().train()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(gamma)); bn.bias.copy_(torch.from_numpy(beta))
        bn.running_mean.copy_(torch.from_numpy(rm)); bn.running_var.copy_(torch.from_numpy(rv))
    xt = torch.from_numpy(x).double().requires_grad_(True)
    wt = torch.from_numpy(w).double().requires_grad_(True)
    zt = F.conv2d(xt, wt, None, padding=(k - 1) // 2, groups=Cin if dw else 1)
    zt.retain_grad()
    yt = F.relu(bn(zt)) if relu else bn(zt)
    gy = rng.normal(size=tuple(yt.shape)).astype(np.float32)
    yt.backward(torch.from_numpy(gy).double())
    xd, wd, gd, bd, rmd, rvd, gyd = (_g(a, dev) for a in (x, w, gamma, beta, rm, rv, gy))
    z, y = torch.full(tuple(zt.shape), float("nan"), device=dev), torch.full(tuple(zt.shape), float("nan"), device=dev)
    stats = torch.full((2 * Cout,), float("nan"), device=dev)
    ops.call("yf_train_unit_forward", 0, xd.data_ptr(), wd.data_ptr(), gd.data_ptr(), bd.data_ptr(), rmd.data_ptr(), rvd.data_ptr(), stats.data_ptr(),
             z.data_ptr(), y.data_ptr(), N, Cin, H, W, Cout, k, 1, dw, relu, ops.scratch)
    tag = "%s relu %d: " % (geom, relu)
    _close(z, zt, 3e-6, tag + "z")
    _close(y, yt, 3e-6, tag + "y")
    mean = zt.detach().mean((0, 2, 3))
    invstd = (zt.detach().var((0, 2, 3), unbiased=False) + 1e-5).rsqrt()
    _close(stats[0::2], mean, 1e-6, tag + "saved mean")
    _close(stats[1::2], invstd, 1e-6, tag + "saved invstd")
    _close(rmd, bn.running_mean, 1e-6, tag + "running_mean")
    _close(rvd, bn.running_var, 1e-6, tag + "running_var")
    dg, db = torch.full((Cout,), float("nan"), device=dev), torch.full((Cout,), float("nan"), device=dev)
    gz, gw, gx = torch.full_like(z, float("nan")), torch.full_like(wd, float("nan")), torch.full_like(xd, float("nan"))
    ops.call("yf_train_unit_backward", 0, xd.data_ptr(), z.data_ptr(), gyd.data_ptr(), stats.data_ptr(), wd.data_ptr(), gd.data_ptr(), bd.data_ptr(),
             dg.data_ptr(), db.data_ptr(), gz.data_ptr(), gw.data_ptr(), gx.data_ptr(), N, Cin, H, W, Cout, k, 1, dw, relu, ops.scratch, ops.scratch_bytes)
    _close(dg, bn.weight.grad, 5e-6, tag + "dgamma")
    _close(db, bn.bias.grad, 5e-6, tag + "dbeta")
    _close(gz, zt.grad, 2e-5, tag + "conv-output gradient (BatchNorm dx)")
    _close(gw, wt.grad, 3e-5, tag + "dw")
    _close(gx, xt.grad, 2e-5, tag + "dx")          # backward data (3e-6) of a conv-output gradient that is itself good to 2e-5
