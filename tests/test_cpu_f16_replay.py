"""The launch-by-launch model of the fp16-storage plan (tests/replay.py, `precision` "f16") and its comparator, without a GPU.

* The model IS the documented one: chained over the whole net, the float32 twin reproduces `oracle.fp16_rounding_sim.Sim(W, T, A, E, size,
  fusion)` bit for bit, on the weights `packer.pack_state_dict` hands the engine.
* Reference against itself: the float32 twin against the float64 replay, launch by launch from the same (the twin's) inputs, over the whole
  parametrisation of tests/test_gpu_f16_replay.py.  Its worst figures per launch kind are the scale of the GPU criteria (replay.REFERENCE_F16),
  and they must themselves stay within the caps: 2 % of a launch's elements, 8 ulps.
* The comparator rejects five deliberate mistakes of the twin under the GPU test's criteria and names the launch.

share = elements that differ from rne16(float64) (chains: further than half an fp16 ulp at the size of the summed terms; heads, fp32: outside
2e-5 of the range); distance = largest |got - float64| in fp16 ulps at max(|float64|, size of the summed terms); see the comparators' comment in
replay.py for why these units.  Measured: twin on the CPU (this file), GPU on an MI355X (test_gpu_f16_replay.py prints its figures).

| launch kind      | kernel                          | twin share | twin dist | GPU share | GPU dist |
|------------------|---------------------------------|-----------:|----------:|----------:|---------:|
| valu             | fused_block_kernel<half_t>      |   0.560 %  |   1.00    |  0.706 %  |   1.00   |
| k19h             | k19h_kernel                     |   0.215 %  |   1.00    |  0.182 %  |   1.00   |
| mres             | mres_kernel / mres_pc_kernel    |   0.273 %  |   1.00    |  0.308 %  |   1.00   |
| mres.wexp        | mres_kernel (conv4_2 written)   |   0.106 %  |   1.00    |  0.104 %  |   1.00   |
| mres.chain       | mres_pc_kernel, nblk 4 / 5      |   0.347 %* |   1.81    |  0.357 %* |   1.13   |
| mres.post        | mres_pc_kernel + conv5_2        |   0.118 %  |   0.50    |  0.059 %  |   0.25   |
| mres.chain.post  | mres_pc_kernel chain + conv5_2  |   0.035 %* |   1.00    |  0.008 %* |   1.00   |
| pw               | pw_mfma_kernel<half_t>          |   0.061 %  |   1.00    |  0.069 %  |   1.00   |
| dcat             | dcat_h_kernel                   |   0.156 %  |   0.50    |  0.151 %  |   0.50   |
| mdw              | mdw_kernel<half_t>              |   0.330 %  |   1.00    |  0.167 %  |   1.00   |
| mdw.head         | mdw_kernel<half_t> + head conv  | 0 %* (1.32 % outside the fp32 criterion) | 0.33 | 0 %* (0.90 %) | 0.33 |
| mdw2             | mdw2_kernel<half_t>             | 0 %* (2.38 %) | 0.41   | 0 %* (4.17 %) | 0.39 |

(* share of elements further than half an fp16 ulp at the terms' size: chains and heads, see replay.by_distance.)  In the result's own
ulps (floor 2^-14) the largest distances are 89 (valu), 2205 (k19h), 619 (mres), 18468 (mres.chain) for the twin and 155, 2197, 494, 24418
for the GPU: cancellation and on-chip rounding flips, not a criterion.  The GPU's shares lie between 0.2 and 1.3 times the twin's: the margin
stays at 3.
"""
import numpy as np
import pytest
import torch

from oracle import backbone_oracle as bo
from oracle.fp16_rounding_sim import Sim, fold
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


def test_weights_are_what_the_packer_hands_the_engine(nets):
    """BatchNorm folded in float64, rounded once to fp32 (packer.fold_bn): the blob's values, which are also Sim's."""
    for sd, net in nets.values():
        fw = fold(sd)
        assert set(fw) == set(net.f32)
        for k, (w, b) in fw.items():
            assert torch.equal(w, net.f32[k][0]) and torch.equal(b, net.f32[k][1]), k


def test_launch_table_has_the_documented_launch_counts():
    """24 launches at 320x256 with fusion 1, 21 with fusion 2; 31 / 29 at 640x512.  Level 0 has no fp16 form."""
    assert [len(rp.launch_table(256, 320, f, "f16")) for f in (1, 2)] == [24, 21]
    assert [len(rp.launch_table(512, 640, f, "f16")) for f in (1, 2)] == [31, 29]
    with pytest.raises(ValueError):
        rp.launch_table(256, 320, 0, "f16")
    for H, W, _ in rp.CASES_F16:
        for f in (1, 2):
            t = rp.launch_table(H, W, f, "f16")
            assert {L.kind for L in t} <= set(rp.KINDS_F16)
            made = {"input"}
            for L in t:                       # every launch reads tensors an earlier launch wrote, every layer runs exactly once
                assert set(L.inputs) <= made, L
                made |= set(L.outputs)
            layers = [l for L in t for l in L.name.split("+")]
            assert sorted(layers) == sorted(rp.LAYER), (H, W, f)


@pytest.mark.parametrize("fusion", [1, 2])
@pytest.mark.parametrize("size", rp.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("weights", WEIGHTS)
def test_chained_twin_is_sim_bit_for_bit(nets, golden, weights, size, fusion):
    sd, net = nets[weights]
    H, W = size
    x = bo.preprocess(rp.frames_u8(golden, H, W, 2))
    t = rp.chained(rp.launch_table(H, W, fusion, "f16"), net, x, "f16")
    hl, hs = Sim(fold(sd), W=True, T=True, A=True, E=True, size=size, fusion=fusion).forward(x)
    assert torch.equal(hl, t["head_large"]) and torch.equal(hs, t["head_small"])
    if size == (256, 352) and fusion == 1:       # no chains, nothing kept on chip: the plan Sim describes by default
        dl, ds = Sim(fold(sd), W=True, T=True, A=True, E=True).forward(x)
        assert torch.equal(hl, dl) and torch.equal(hs, ds)


@pytest.fixture(scope="module")
def measured(nets, golden):
    """{(weights, H, W, N, fusion): [(launch, out_name, Cmp, share)]}: the twin against the float64 replay, per launch."""
    out = {}
    for wname in WEIGHTS:
        net = nets[wname][1]
        for H, W, N in rp.CASES_F16:
            x = bo.preprocess(rp.frames_u8(golden, H, W, N))
            for fusion in (1, 2):
                table = rp.launch_table(H, W, fusion, "f16")
                t = rp.chained(table, net, x, "f16")
                out[(wname, H, W, N, fusion)] = [(L, n, c, s) for L in table for n, c, s, _ in rp.replay_and_check(L, net, t, t, "f16")]
    return out


def _worst(measured):
    w = {}
    for rows in measured.values():
        for L, n, c, s in rows:
            a = w.setdefault(L.kind, [0.0, 0.0, 0.0, 0.0])
            a[0], a[1], a[2], a[3] = max(a[0], s), max(a[1], c.dist), max(a[2], c.ulps), max(a[3], c.share if L.fp32_out else 0.0)
    return w


def test_reference_against_itself_stays_within_the_caps(measured):
    bad = ["%s %s -> %s: share %.3f %%, distance %.2f; %s" % (key, L.name, n, 100 * s, c.dist, c.where)
           for key, rows in measured.items() for L, n, c, s in rows if s > rp.SHARE_CAP or c.dist > rp.ULP_CAP]
    assert not bad, "\n".join(bad)


def test_reference_figures_are_the_recorded_ones(measured):
    """replay.REFERENCE_F16 is what the GPU criteria are multiples of: every kind is exercised, nothing measured here exceeds its entry,
    and no entry is more generous than the measurement (a quarter of slack for another torch build's summation order)."""
    w = _worst(measured)
    for k in sorted(w):
        print("%-16s share %.4f %%  distance %.3f  (in the result's own ulps: %.0f; outside the fp32 criterion %.3f %%)   recorded %s %s"
              % (k, 100 * w[k][0], w[k][1], w[k][2], 100 * w[k][3], rp.REFERENCE_F16.get(k), rp.F32_REFERENCE_F16.get(k)))
    assert set(w) == set(rp.KINDS_F16) == set(rp.REFERENCE_F16)
    for k, (s, d, _, f) in w.items():
        if k in rp.F32_REFERENCE_F16:
            assert f <= rp.F32_REFERENCE_F16[k] <= 1.25 * f + 1e-5, (k, f)
        else:
            assert f == 0.0
        rs, rd = rp.REFERENCE_F16[k]
        assert s <= rs and d <= rd, (k, s, d)
        assert rs <= 1.25 * s + 1e-5 and rd <= 1.25 * d + 0.05, (k, s, d)
        assert rs <= rp.SHARE_CAP / rp.MARGIN or rp.limits(k, rp.REFERENCE_F16)[0] == rp.SHARE_CAP


# ---- the comparator ------------------------------------------------------------------------------------------------------------------

def test_comparator_counts_and_units():
    e = torch.zeros(2, 3, 4, 5, dtype=torch.float64) + 1.0
    g = e.clone().float()
    c = rp.compare(g, e)
    assert (c.share, c.far, c.dist, c.n_diff, c.where) == (0.0, 0.0, 0.0, 0, "")
    g[1, 2, 3, 4] += 2.0 ** -10                              # one ulp of 1.0, last row and column of frame 1
    g[0, 0, 1, 1] += 2.0 ** -12                              # a quarter of an ulp: still not the rounded exact value
    c = rp.compare(g, e, tiles=((2, 5),))
    assert c.n_diff == 2 and c.share == 2 / 120 and c.dist == 1.0 and c.far == 1 / 120
    assert "(n=1, c=2, y=3, x=4)" in c.where and "border" in c.where and "per frame [1, 1]" in c.where and "last column 1, last row 1" in c.where
    e2 = e * 2.0 ** -20                                       # below the smallest normal: the unit stays 2^-24
    assert rp.compare(e2.float() + 2.0 ** -24, e2).dist == 1.0
    scale = torch.full_like(e, 1024.0)                        # the element is a 1024th of its terms: unit = ulp16(1024) = 1
    c = rp.compare(g, e, scale)
    assert c.dist == 2.0 ** -10 and c.ulps == 1.0 and c.far == 0.0 and c.n_diff == 2
    c = rp.compare(g, e, fp32=True)                           # fp32 outputs: 2e-5 of the range
    assert c.n_diff == 2 and rp.compare(e.float() + 1e-5, e, fp32=True).n_diff == 0


MISTAKES = {
    # what the twin does wrong                                        -> the launch that must be named
    "tap_dropped_on_the_last_column": (dict(drop_tap=dict(layer="conv3_3", ky=0, kx=1)), "conv3_2+conv3_3+conv3_4"),
    "a_rounding_of_a_projection_skipped": (dict(skip_a="res3_3.conv3"), "res3_3.conv1+res3_3.conv2+res3_3.conv3"),
    "bias_added_after_the_output_rounding": (dict(late_bias="conv4_1"), "conv3_5+conv3_6+conv4_1"),
    "two_channels_of_conv1_8_swapped": (dict(swap_channels=dict(pair=(3, 17))), "conv1_8+conv1_9+conv2_1"),
    "bottom_halo_row_of_frame_1_from_frame_0": (dict(halo_frame=dict(layer="res2_1.conv2", tile_h=16)), "res2_1.conv1+res2_1.conv2+res2_1.conv3"),
}


@pytest.mark.parametrize("mistake", list(MISTAKES))
def test_comparator_rejects_a_subtly_wrong_twin_and_names_the_launch(nets, golden, mistake):
    """The smallest size, two frames, shipped weights, the GPU test's criteria.  Every launch of the twin runs from the correct twin's tensors
    with the mistake switched on: all launches but one give the correct twin's bits (which pass: test_reference_against_itself), and that one
    is rejected against the float64 replay of the same launch, in a message that names it."""
    perturb, launch_name = MISTAKES[mistake]
    H, W, N = rp.CASES_F16[0]
    net = rp.Net(nets["shipped"][0])
    x = bo.preprocess(rp.frames_u8(golden, H, W, N))
    table = rp.launch_table(H, W, 1, "f16")
    clean = rp.chained(table, net, x, "f16")
    assert not [v for L in table for n, c, s, v in rp.replay_and_check(L, net, clean, clean, "f16", rp.REFERENCE_F16) if v]
    net.perturb = perturb
    wrong = []
    for L in table:
        got = rp.run(L, net, clean, "f16")
        if all(torch.equal(got[n], clean[n]) for n in got):
            continue
        wrong.append(L.name)
        verdicts = [v for n, c, s, v in rp.replay_and_check(L, net, clean, got, "f16", rp.REFERENCE_F16)]
        assert all(verdicts) and all(("launch " + L.name) in v for v in verdicts), verdicts
        print(verdicts[0])
    assert wrong == [launch_name]
