"""The launch-by-launch replay of the fp32-storage plans (tests/replay.py: `f32` and `f16x3` engines, fusion 0 / 1 / 2), without a GPU.

* The model IS the reference's graph: the float64 launches chained over the whole net equal `backbone_oracle.forward` on the float64
  state dict to 1e-12 of the range, at every fusion level and two sizes.
* The twin against the replay: the CPU twin of each precision (torch float32; for f16x3 the split operands and the three products the
  kernels issue) against the float64 replay, launch by launch from the twin's own tensors, over the whole parametrisation of
  tests/test_gpu_plan_replay.py.  The worst distance per (precision, launch kind) is `replay.REFERENCE_F32`; the GPU is held to 3 x that, and
  never to more than the launch's a-priori bound (the cap), inside which the twin itself must lie.
* Planted defects of the twin are rejected under the GPU test's criteria and attributed to their launch; for each it is recorded whether the
  head-level rule (tests/test_gpu_parity.py `_check_heads`: 3 x torch's own fp32 error, 86 layers downstream) would have caught it.

distance = largest |got - float64| in fp32 ulps at max(|float64|, M), M = sum |w| |x| + |b| (+ |residual|) of the launch's last conv.
Measured: twin on the CPU (this file), GPU on an MI355X (tests/test_gpu_plan_replay.py prints its figures).  cap = the sum over the launch's
layers of the terms an output sums (x 4 for a split-operand GEMM), smallest and largest launch of the kind; "prop." = propagated per element
(replay.PROPAGATED_CAP has the reason), with the largest share of that bound used by twin / GPU.

| launch kind      | kernel (f32 / f16x3)                          | f32 twin | f32 GPU | x3 twin | x3 GPU | cap f32 / x3           |
|------------------|-----------------------------------------------|---------:|--------:|--------:|-------:|------------------------|
| valu.stem        | fused_block_kernel<float>, conv0 in front     |  2920.89 | 2749.93 | 2920.89 | 2749.93 | prop. (0.022, 0.019) / prop. (0.022, 0.019) |
| valu             | fused_block_kernel<float>                     |    24.12 |   22.94 |   12.16 |  22.94 | prop. (0.074, 0.071) / prop. (0.065, 0.065) |
| k19r             | k19r_kernel / -                               |     4.81 |    6.54 |       - |      - | 247 / - |
| k19m             | - / k19m_kernel                               |        - |       - |   13.12 |  13.06 | - / 973 |
| mres             | mres_kernel, mres_pc_kernel <float / x3_t>    |     6.14 |    5.54 |    8.33 |   7.67 | 52 .. 285 / 178 .. 1110 |
| mres.wexp        | mres_kernel (conv4_2 written)                 |     4.50 |    4.73 |    7.72 |   6.01 | 172 / 658 |
| mres.chain       | mres_pc_kernel, nblk 4 / 5                    |    11.73 |   13.06 |   13.82 |  13.69 | 692 .. 1425 / 2648 .. 5550 |
| mres.unchained   | launch_chain_unchained, 4 dispatches          |     9.89 |   11.14 |   12.63 |  12.08 | 692 / 2648 |
| mres.esplit      | mres_esplit_kernel, 6 dispatches / -          |     8.49 |    5.90 |       - |      - | 1425 / - |
| mres.esplit.post | mres_esplit_kernel + conv5_2 / -              |     4.66 |    4.83 |       - |      - | 1474 / - |
| mres.post        | mres_pc_kernel + conv5_2                      |     3.41 |    3.66 |    3.23 |   4.50 | 334 / 1159 |
| mres.chain.post  | mres_pc_kernel chain + conv5_2                |     4.66 |    4.83 |    5.83 |   5.88 | 1474 / 5599 |
| pw               | pw_ws_kernel / pw_ws_x3_kernel                |     5.76 |    6.96 |    7.34 |   6.62 | 49 .. 233 / 196 .. 932 |
| dcat             | dcat_kernel / dcat_x3_kernel                  |     5.74 |    6.93 |    5.23 |   6.92 | 330 / 1320 |
| mdw              | mdw_kernel                                    |     5.84 |    5.46 |    7.37 |   7.21 | 123 / 414 |
| mdw.head         | mdw_kernel + head conv                        |     5.78 |    5.92 |    6.16 |   3.94 | 220 .. 284 / 802 .. 1058 |
| mdw2             | mdw2_kernel                                   |     5.48 |    6.06 |    4.51 |   3.26 | 407 / 1472 |
| mdw2.esplit      | mdw2_esplit_kernel, 3 dispatches / -          |     5.30 |    6.06 |       - |      - | 407 / - |
| l.dense          | dense3x3s2 (fusion 0)                         |     3.35 |    5.02 |    3.35 |   5.02 | 10 .. 217 / 10 .. 217 |
| l.pw             | launch_pw, VALU (fusion 0)                    |     6.96 |    7.04 |    6.96 |   7.04 | 5 .. 233 / 5 .. 233 |
| l.dw             | launch_dw (fusion 0)                          |     4.25 |    3.99 |    4.25 |   3.99 | 10 .. 26 / 10 .. 26 |
| l.dc             | launch_pw deconv (fusion 0)                   |     3.74 |    5.08 |    3.74 |   5.08 | 97 / 97 |
| l.head           | launch_pw head (fusion 0)                     |     5.60 |    5.17 |    5.60 |   5.17 | 97 .. 129 / 97 .. 129 |

The GPU's worst distances lie between 0.6 and 1.9 times the twin's (1.9: `valu` in an f16x3 engine, the same fp32 kernel as in an f32 engine,
measured against a twin figure that lacks the 256x320 cases); the margin stays at 3.  The f16x3 figures are those of fp32: the split operands
keep 22 bits and the twin, which models exactly the three products, is as far from float64 as the fp32 twin.  In the results' own ulps the
distances reach 10^6 and more in every kind (an output that is a millionth of its terms): not a criterion.

Planted defects (96x160, N = 2, fusion 1, shipped weights; distance against the launch's limit; head-level rule):
  tap dropped on the last column (conv3_3)              f32    7469327.5 / 18.8   caught by the head-level rule too
  bottom halo row of frame 1 from frame 0 (res2_1)      f32  234186625.3 / 73.8   caught too
  one 3x3 depthwise tap 1e-5 off, last column (res3_3)  f32         41.6 / 18.8   PASSED by the head-level rule
  one 5x5 depthwise tap 1e-5 off, last column (conv4_1_2) x3        50.8 / 22.6   PASSED by the head-level rule
  bias rounded to fp16 (conv4_1 / res3_3.conv3)         f32, x3   1802.2 / 18.8, 1984.0 / 25.5   caught too
  w_lo a_hi left out (res3_4.conv3 / conv5_2)           x3        2452.3 / 25.5, 2148.7 / 22.5   caught too
  subnormal lo halves flushed (conv1_9 / res5_3.conv1)  x3        4310.4 / 40.2, 1387.1 / 42.3   caught too
  lo = 0 for operands below 2^-14                       x3        the launch's bits do not change: not a defect (last test of this file)
"""
import numpy as np
import pytest
import torch

from oracle import backbone_oracle as bo
from tests import replay as rp

WEIGHTS = ("shipped", "random")
rp.cap_threads()


@pytest.fixture(scope="module")
def nets():
    out = {}
    for k, load in rp.state_dicts().items():
        sd = load()
        out[k] = (sd, rp.Net(sd))
    return out


@pytest.mark.parametrize("fusion", [0, 1, 2])
@pytest.mark.parametrize("size", [(96, 160), (160, 224)], ids=lambda s: "%dx%d" % s)
def test_float64_launches_chain_to_the_reference_graph(nets, golden, size, fusion):
    sd = nets["shipped"][0]
    H, W = size
    x = bo.preprocess(rp.frames_u8(golden, H, W, 2)).double()
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    ref = bo.forward(sd64, x)
    for precision in rp.FP32_STORAGE:          # the float64 evaluation does not depend on the engine; the table's structure does
        t = rp.chained(rp.launch_table(H, W, fusion, precision, N=2), rp.Net64(sd), x, precision, "exact")
        for got, want in ((t["head_large"], ref[0]), (t["head_small"], ref[1])):
            assert got.dtype == torch.float64
            assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_launch_table_counts_dtypes_and_forms():
    """24 launches at 320x256 with fusion 1, 21 with fusion 2 (the headline's), 31 / 29 at 640x512; one per layer at
    level 0.  Every launch reads tensors an earlier one wrote, every layer runs once; dtypes as build_plan / yf_create_ex hand them out; each
    case reaches the forms it exists for on a 256-CU device."""
    for p in rp.FP32_STORAGE:
        assert [len(rp.launch_table(256, 320, f, p, N=256)) for f in (0, 1, 2)] == [len(bo.LAYERS) + 2, 24, 21]
        assert [len(rp.launch_table(512, 640, f, p, N=256)) for f in (1, 2)] == [31, 29]
    kinds = set()
    for H, W, N, fusions, precisions in rp.CASES_F32:
        for f in fusions:
            for p in precisions:
                t = rp.launch_table(H, W, f, p, N=N)
                made = {"input"}
                for L in t:
                    assert set(L.inputs) <= made, L
                    made |= set(L.outputs)
                    kinds.add((p, L.kind))
                    assert L.terms > 0
                assert sorted(l for L in t for l in L.name.split("+")) == sorted(rp.LAYER), (H, W, f)
                if f == 0:
                    assert {L.dtype for L in t} == {rp.DT["f32"]}                      # an x3 engine hands every per-layer op DT_F32
                    assert {L.dispatches for L in t} == {1}
                elif p == "f16x3":
                    assert {L.dtype for L in t if L.kind.startswith("valu")} == {rp.DT["f32"]}
                    assert {L.dtype for L in t if not L.kind.startswith("valu")} == {rp.DT["f16x3"]}
                else:
                    assert {L.dtype for L in t} == {rp.DT["f32"]}
                fm = rp.forms(t)
                want = rp.expect(H, W, N, f, p, 256)
                assert f == 0 or want
                for name, (kind, disp) in want.items():
                    assert fm[name][:2] == (kind, disp), (H, W, N, f, p, name, fm[name])
    assert kinds == set(rp.REFERENCE_F32)
    # the forms the cases exist for, all reached: the esplit pair and the first batch that leaves it are fp32 only
    assert {k for p, k in kinds if p == "f32"} - {k for p, k in kinds if p == "f16x3"} == {"k19r", "mres.esplit", "mres.esplit.post", "mdw2.esplit"}
    assert {k for p, k in kinds if p == "f16x3"} - {k for p, k in kinds if p == "f32"} == {"k19m"}
    few, many = rp.forms(rp.launch_table(160, 224, 2, "f32", N=2)), rp.forms(rp.launch_table(160, 224, 2, "f32", N=36))
    # stride 16 at 160x224 is one tile per frame: 36 frames are still few there.  The 16x20 form of the stride-16 mdw pair is reached at
    # 96x160 (launch_mdw: `a.H > 8`), dcat's five-tile items at 96x160, N = 132
    small, big = rp.forms(rp.launch_table(96, 160, 2, "f32", N=2)), rp.forms(rp.launch_table(96, 160, 2, "f32", N=132))
    assert few["conv4_1_2+conv4_1_3"][2] == many["conv4_1_2+conv4_1_3"][2] == "8x10" and small["conv4_1_2+conv4_1_3"][2] == big["conv4_1_2+conv4_1_3"][2] == "16x20"
    assert small["deconv5_1+conv4_1_1"][2].startswith("one") and big["deconv5_1+conv4_1_1"][2].startswith("five")
    assert small["conv1_8+conv1_9+conv2_1"][2] == "8 waves" and rp.forms(rp.launch_table(256, 320, 2, "f32", N=256))["conv1_8+conv1_9+conv2_1"][2].startswith("16 waves")
    assert few["+".join(rp.res_block("res3_3"))][2] == "8x10" and many["+".join(rp.res_block("res3_3"))][2] == "16x20"
    assert few["+".join(rp.res_block("res2_1"))][2] == "16x16" and many["+".join(rp.res_block("res2_1"))][2] == "32x16"
    assert few["conv3_5+conv3_6+conv4_1"][2] == "8x4" and many["conv3_5+conv3_6+conv4_1"][2] == "8x10"


@pytest.fixture(scope="module")
def measured(nets, golden):
    """{(weights, H, W, N, fusion, precision): [(launch, out_name, Dist)]}: the twin against the float64 replay, per launch."""
    out = {}
    for wname in WEIGHTS:
        net = nets[wname][1]
        for H, W, N, fusions, precisions in rp.CASES_F32:
            if wname == "shipped" and (H, W, N) in rp.RANDOM_ONLY:
                continue
            x = bo.preprocess(rp.frames_u8(golden, H, W, N))
            for f in fusions:
                for p in precisions:
                    table = rp.launch_table(H, W, f, p, N=N)
                    t = rp.chained(table, net, x, p)
                    out[(wname, H, W, N, f, p)] = [(L, n, d) for L in table for n, d, _ in rp.replay_and_check(L, net, t, t, p)]
    return out


def test_twin_figures_are_the_recorded_ones(measured):
    """replay.REFERENCE_F32 is what the GPU criteria are multiples of: every (precision, kind) is exercised, nothing measured here exceeds
    its entry, and no entry is more generous than the measurement (a quarter of slack for another torch build's summation order)."""
    w, caps, used = {}, {}, {}
    for (wname, H, W, N, f, p), rows in measured.items():
        for L, n, d in rows:
            k = (p, L.kind)
            w[k] = max(w.get(k, 0.0), d.dist)
            caps[k] = (min(caps.get(k, (1e30, 0))[0], rp.cap(L)), max(caps.get(k, (1e30, 0))[1], rp.cap(L)))
            used[k] = max(used.get(k, 0.0), d.cap_used)
    for k in sorted(w):
        print("%-6s %-18s twin %8.2f   recorded %8.2f   cap %s, largest share used %.3f" % (
            k[0], k[1], w[k], rp.REFERENCE_F32.get(k, float("nan")), "propagated" if k[1] in rp.PROPAGATED_CAP else "%.0f .. %.0f" % caps[k], used[k]))
    assert set(w) == set(rp.REFERENCE_F32)
    for k, d in w.items():
        assert d <= rp.REFERENCE_F32[k] <= 1.25 * d + 0.05, (k, d)


def test_twin_stays_inside_the_cap(measured):
    """The cap is a condition on the limits: min(3 x twin, cap).  It must not cut into the twin itself -- where it does, the model of that
    kind is wrong or the cap needs a stated reason.  It does in the fp32 VALU block launches only, for the reason written at
    replay.PROPAGATED_CAP: their cap is the propagated bound, and the twin stays inside THAT everywhere."""
    outside = set()
    for key, rows in measured.items():
        for L, n, d in rows:
            assert np.isfinite(d.dist)
            if L.kind in rp.PROPAGATED_CAP:
                assert d.cap_used <= 1.0, (key, L.name, n, d)
                if d.dist > L.terms:
                    outside.add(L.kind)
            else:
                assert d.dist <= rp.cap(L) and d.cap_used <= 1.0, (key, L.name, n, d.dist, rp.cap(L))
    assert outside == {"valu.stem"}           # over the parametrisation; `valu`: the next test


def test_res1_1_leaves_the_sum_of_terms_with_the_shipped_weights(nets, golden):
    """Why `valu` has the propagated cap although the twin uses 24.1 of 25 over the parametrisation: with the shipped weights at 160x224,
    N = 36 (a batch the parametrisation runs with random weights only) res1_1 is 28.5 ulps from float64."""
    net = nets["shipped"][1]
    x = bo.preprocess(rp.frames_u8(golden, 160, 224, 36))
    table = rp.launch_table(160, 224, 1, "f32", N=36)[:2]
    t = rp.chained(table, net, x, "f32")
    (n, d, _), = rp.replay_and_check(table[1], net, t, t, "f32")
    print("res1_1: %.2f ulps, sum of terms %.0f, share of the propagated bound %.3f" % (d.dist, table[1].terms, d.cap_used))
    assert table[1].kind == "valu" and d.dist > table[1].terms and d.cap_used <= 1.0


def test_distance_units():
    e = torch.ones(2, 3, 4, 5, dtype=torch.float64)
    g = e.clone().float()
    m = torch.zeros_like(e)
    assert rp.distance(g, e, m).dist == 0.0
    g[1, 2, 3, 4] += 2.0 ** -23                              # one fp32 ulp of 1.0, last row and column of frame 1
    d = rp.distance(g, e, m, tiles=((2, 5),), limit=0.5)
    assert d.dist == 1.0 and d.own == 1.0
    assert "(n=1, c=2, y=3, x=4)" in d.where and "border" in d.where and "per frame [0, 1]" in d.where and "last column 1, last row 1" in d.where
    assert rp.distance(g, e, m, limit=1.0).where == ""        # at the limit: passes
    assert rp.distance(g, e, torch.full_like(e, 1024.0)).dist == 2.0 ** -10     # the element is a 1024th of its terms
    b = torch.full_like(e, 2.0 ** -24)                        # a propagated bound of half an ulp: tighter than the limit, and exceeded
    d = rp.distance(g, e, m, limit=4.0, bound64=b)
    assert d.cap_used == 2.0 and "(n=1, c=2, y=3, x=4)" in d.where
    assert rp.distance(g, e, m, limit=4.0, bound64=b * 4).where == ""
    g[0, 0, 0, 0] = float("inf")
    with pytest.raises(AssertionError, match="non-finite"):
        rp.distance(g, e, m)
    assert rp.ulp32(np.array([1.0, 1.5, 2.0, 0.75]))[:].tolist() == [2.0 ** -23, 2.0 ** -23, 2.0 ** -22, 2.0 ** -24]


DEFECTS = {
    # what the twin does wrong                         precision  perturbation                                          the launch that must be named
    "tap_dropped_on_the_last_column": ("f32", dict(drop_tap=dict(layer="conv3_3", ky=0, kx=1)), "conv3_2+conv3_3+conv3_4"),
    "bottom_halo_row_of_frame_1_from_frame_0": ("f32", dict(halo_frame=dict(layer="res2_1.conv2", tile_h=16)), "res2_1.conv1+res2_1.conv2+res2_1.conv3"),
    "one_depthwise_tap_1e-5_off_on_the_last_column": ("f32", dict(tap_scale=dict(layer="res3_3.conv2", ky=1, kx=1, rel=1e-5)),
                                                      "res3_3.conv1+res3_3.conv2+res3_3.conv3"),
    "one_5x5_tap_1e-5_off_on_the_last_column_x3": ("f16x3", dict(tap_scale=dict(layer="conv4_1_2", ky=2, kx=2, rel=1e-5)), "conv4_1_2+conv4_1_3"),
    "bias_rounded_to_fp16": ("f32", dict(bias16="conv4_1"), "conv3_5+conv3_6+conv4_1"),
    "bias_rounded_to_fp16_x3": ("f16x3", dict(bias16="res3_3.conv3"), "res3_3.conv1+res3_3.conv2+res3_3.conv3"),
    "x3_lo_hi_product_left_out": ("f16x3", dict(no_lo_hi="res3_4.conv3"), "res3_4.conv1+res3_4.conv2+res3_4.conv3"),
    "x3_lo_hi_product_left_out_in_conv5_2": ("f16x3", dict(no_lo_hi="conv5_2"), "conv5_2"),
    "x3_subnormal_lo_halves_flushed": ("f16x3", dict(flush_subnormal_lo="conv1_9"), "conv1_8+conv1_9+conv2_1"),
    "x3_subnormal_lo_halves_flushed_in_a_chain": ("f16x3", dict(flush_subnormal_lo="res5_3.conv1"), rp.RES5),
}


@pytest.fixture(scope="module")
def clean(nets, golden):
    """The smallest size, two frames, fusion 1, shipped weights: the correct twins' tensors, the references of the head-level rule."""
    sd = nets["shipped"][0]
    H, W, N = 96, 160, 2
    x = bo.preprocess(rp.frames_u8(golden, H, W, N))
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    out = dict(x=x, ref64=bo.forward(sd64, x.double()), ref32=bo.forward(sd, x))
    for p in rp.FP32_STORAGE:
        table = rp.launch_table(H, W, 1, p, N=N)
        t = rp.chained(table, rp.Net(sd), x, p)
        assert not [v for L in table for n, d, v in rp.replay_and_check(L, rp.Net(sd), t, t, p) if v]
        assert rp.heads_rule(t["head_large"], t["head_small"], out["ref32"], out["ref64"])
        out[p] = (table, t)
    return out


@pytest.fixture(scope="module")
def planted(nets, clean):
    """Per defect: every launch of the twin runs from the correct twin's tensors with the defect switched on; the launches whose bits change,
    their verdicts under the GPU test's criteria, and the head-level rule applied to the chained twin with the defect."""
    out = {}
    for defect, (precision, perturb, launch_name) in DEFECTS.items():
        table, good = clean[precision]
        net = rp.Net(nets["shipped"][0])
        net.perturb = perturb
        wrong, verdicts, dist, lim = [], [], 0.0, 0.0
        for L in table:
            got = rp.run(L, net, good, precision)
            if all(torch.equal(got[n], good[n]) for n in got):
                continue
            wrong.append(L.name)
            res = rp.replay_and_check(L, net, good, got, precision)
            verdicts += [v for n, d, v in res if v]
            dist, lim = max(d.dist for n, d, v in res), rp.limit(precision, L)
        t = rp.chained(table, net, clean["x"], precision)
        caught = not rp.heads_rule(t["head_large"], t["head_small"], clean["ref32"], clean["ref64"])
        out[defect] = (wrong, verdicts, dist, lim, caught)
    return out


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_planted_defect_is_rejected_and_attributed(planted, defect):
    """All launches but one give the correct twin's bits, and that one is rejected against the float64 replay of the same launch in a
    message that names it."""
    precision, perturb, launch_name = DEFECTS[defect]
    wrong, verdicts, dist, lim, caught = planted[defect]
    assert wrong == [launch_name]
    assert verdicts and all(("launch " + launch_name + " [") in v for v in verdicts), verdicts
    print("%-48s %-6s distance %12.1f  limit %6.1f  head-level rule: %s" % (defect, precision, dist, lim, "catches it" if caught else "PASSES IT"))


def test_some_defect_is_caught_by_the_replay_only(planted):
    """How large the gap was: would the suite have noticed without the replay?  The head-level rule passes a depthwise tap that is 1e-5 off
    on the last column (both precisions); everything else planted here is gross enough to show 86 layers downstream at this size."""
    missed = sorted(k for k, r in planted.items() if not r[4])
    assert missed == ["one_5x5_tap_1e-5_off_on_the_last_column_x3", "one_depthwise_tap_1e-5_off_on_the_last_column"]


def test_lo_of_an_operand_below_the_smallest_normal_is_zero_anyway(nets, clean):
    """'lo taken as 0 for operands below 2^-14' is no defect: such an operand's hi is an fp16 subnormal (spacing 2^-24), a - hi is at most
    2^-25 and rounds to zero (ties to even), so the launch's bits do not change.  What an MFMA that flushed subnormals would lose is the lo
    half of every operand below 1/8, whose lo is itself subnormal: DEFECTS' x3_subnormal_lo_halves_flushed, thousands of ulps."""
    table, good = clean["f16x3"]
    net = rp.Net(nets["shipped"][0])
    for layer in ("conv1_9", "conv5_2", "res5_3.conv1", "head_4"):
        net.perturb = dict(flush_lo=layer)
        for L in table:
            got = rp.run(L, net, good, "f16x3")
            assert all(torch.equal(got[n], good[n]) for n in got), (layer, L.name)
