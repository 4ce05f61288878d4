"""oracle/train_replay.py on the CPU: the replay model is exact, torch's own fp32 backward passes the acceptance rule against it, and
the rule rejects the defects it exists to catch.  (The GPU side is tests/test_gpu_train_replay.py.)

Setting: N = 3 frames of 64x96, the random weights of tests/random_weights.py (BatchNorm biases away from zero, so ReLU masks are not
sign-symmetric), random head gradients.  Measured, per tensor relative to its largest element, seed 1 / seed 2:
  torch fp32 gradients vs the plain from-the-input float64 oracle        median 4.2e-3 / 9.6e-3, 90th percentile 6.5e-3 / 1.8e-2
  the same gradients vs the float64 replay on their own tape             median 8.5e-7 / 6.8e-7, 90th percentile 1.7e-6 / 1.4e-6, max 4.6e-6 / 6.8e-6
so a tensor that is off by 1e-4 cannot hide.  With the frames fed in another order (another summation order) the worst tensor is at 1.7x
of max(its twin's error, the twin's median); the rule allows 8x.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import backbone_oracle as bo  # noqa: E402
from oracle import train_replay as tr  # noqa: E402

N, H, W = 3, 64, 96
# BatchNorm biases of the units WITHOUT ReLU: a shift of such a unit's output is a per-channel constant at the input of whatever follows.
NO_RELU_BIASES = sorted(l[0] + ".1.bias" for l in bo.LAYERS if not l[6])
# Where every consumer is a pointwise conv + train-mode BatchNorm the shift drops out of the batch-normalised output, and the gradient
# is ZERO in exact arithmetic (1e-11 .. 1e-15 in the float64 replay, against 3 .. 4e4 for every other tensor).  Four of the 27 are not in
# that position: conv5_4 and conv4_1_3 feed a padded 5x5 depthwise conv (the shift is not constant at the border), conv5_6 and conv4_1_5
# feed a head, which has no BatchNorm.  Their gradients are O(1) and they ARE compared: the zero set is these 23, fewer than the 27 allowed.
ZERO_SET = sorted(set(NO_RELU_BIASES) - {"conv5_4.1.bias", "conv5_6.1.bias", "conv4_1_3.1.bias", "conv4_1_5.1.bias"})


def _case(seed):
    from random_weights import random_state_dict
    sd0 = random_state_dict(seed)
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((N, 1, H, W), generator=g) - 0.5
    return sd0, x, torch.randn((N, 24, H // 16, W // 16), generator=g), torch.randn((N, 24, H // 32, W // 32), generator=g)


def _plain(sd0, x, g_hl, g_hs, dtype):
    """torch.autograd.grad of the plain oracle, from the input."""
    sd = bo.training_state(sd0, dtype)
    keys = bo.parameter_keys(sd)
    heads = bo.forward(sd, x.to(dtype), train=True)
    return dict(zip(keys, torch.autograd.grad(list(heads), [sd[k] for k in keys], [g_hl.to(dtype), g_hs.to(dtype)])))


_CACHE = {}


def _standin(seed):
    """An fp32 run of the oracle standing in for the device: its tape, its gradients, the float64 replay and the fp32 twin of that tape."""
    if seed not in _CACHE:
        sd0, x, g_hl, g_hs = _case(seed)
        _, _, tape = tr.make_tape(sd0, x, torch.float32)
        g64, fwd = tr.replay(sd0, tape, g_hl, g_hs, torch.float64)
        g_twin, _ = tr.replay(sd0, tape, g_hl, g_hs, torch.float32)
        _CACHE[seed] = dict(sd0=sd0, x=x, g_hl=g_hl, g_hs=g_hs, tape=tape, g64=g64, fwd=fwd, g_twin=g_twin)
    return _CACHE[seed]


def test_replay_of_a_float64_tape_is_the_plain_backward():
    """A float64 tape made by the oracle itself, replayed in float64, IS torch.autograd.grad of the plain oracle (1e-10 of each tensor's
    largest element; the zero set against the largest gradient) -- for the whole network and for the subset from res4_1.conv1 on, whose
    downstream gradient is the full run's."""
    sd0, x, g_hl, g_hs = _case(1)
    want = _plain(sd0, x, g_hl, g_hs, torch.float64)
    hl, hs, tape = tr.make_tape(sd0, x, torch.float64)
    sd = bo.training_state(sd0, torch.float64)
    heads = bo.forward(sd, x.double(), train=True)
    assert torch.equal(hl, heads[0].detach()) and torch.equal(hs, heads[1].detach())
    assert sorted(tape) == sorted(tr.unit_names() + ["head_4", "head_5"])
    top = max(float(v.abs().max()) for v in want.values())
    got, fwd = tr.replay(sd0, tape, g_hl, g_hs, torch.float64)
    assert list(got) == tr.parameter_keys() and sorted(got) == sorted(want) and len(got) == 256
    for k in want:
        assert float((got[k] - want[k]).abs().max()) <= 1e-10 * max(float(want[k].abs().max()), 1e-9 * top), k
    assert max(max(e) for e in fwd.values()) <= 1e-12          # the tape's z and y are what the replay computes from the tape's x
    sub, fwd_sub = tr.replay(sd0, tape, g_hl, g_hs, torch.float64, first_unit="res4_1.conv1")
    assert list(sub) == tr.parameter_keys("res4_1.conv1") and len(sub) == 127 and "conv4_1.1.bias" not in sub
    assert list(fwd_sub) == tr.unit_names("res4_1.conv1")
    for k in sub:
        assert float((sub[k] - want[k]).abs().max()) <= 1e-10 * max(float(want[k].abs().max()), 1e-9 * top), k
    with pytest.raises(ValueError):
        tr.replay(sd0, tape, g_hl, g_hs, torch.float64, first_unit="res4_1.conv2")


@pytest.mark.parametrize("seed", [1, 2])
def test_torch_fp32_passes_against_its_own_twin(seed):
    """torch's fp32 backward from the input (the device's stand-in) against the float64 replay of its own tape, judged by compare()
    with the fp32 replay as twin; then the same with the frames fed in another order, which is another summation order in every BatchNorm
    and weight-gradient sum (what the device's tiles and slabs amount to) -- that one is not bit-equal to the twin and has to fit the
    margins.  The zero set is pinned, and the tape's forward errors are at fp32 rounding."""
    c = _standin(seed)
    g32 = _plain(c["sd0"], c["x"], c["g_hl"], c["g_hs"], torch.float32)
    r = tr.compare(g32, c["g64"], c["g_twin"])
    print("\n[replay, seed %d] %s" % (seed, r.table()))
    assert r.ok, r.failures
    assert sorted(r.zero) == ZERO_SET and len(ZERO_SET) == 23 and set(ZERO_SET) <= set(NO_RELU_BIASES) and len(NO_RELU_BIASES) == tr.ZERO_CAP
    f = r.figures()
    assert f["twin_p90"] <= 5e-6 and f["twin_max"] <= 2e-5, f      # the yardstick itself is at rounding level: 1e-4 cannot pass
    assert max(e[0] for e in c["fwd"].values()) <= 3e-6 and max(e[1] for e in c["fwd"].values()) <= 3e-6
    perm = torch.tensor([2, 0, 1])
    inv = torch.argsort(perm)
    gp = _plain(c["sd0"], c["x"][perm], c["g_hl"][perm], c["g_hs"][perm], torch.float32)
    _, _, tape_p = tr.make_tape(c["sd0"], c["x"][perm], torch.float32)
    tape_p = {k: (v[inv] if torch.is_tensor(v) else (v[0][inv], v[1][inv], v[2][inv]) + v[3:]) for k, v in tape_p.items()}
    g64p, _ = tr.replay(c["sd0"], tape_p, c["g_hl"], c["g_hs"], torch.float64)
    twin_p, _ = tr.replay(c["sd0"], tape_p, c["g_hl"], c["g_hs"], torch.float32)
    rp = tr.compare(gp, g64p, twin_p)
    print("[replay, seed %d, frames permuted] %s" % (seed, rp.table()))
    assert any(not torch.equal(gp[k], twin_p[k]) for k in gp)
    assert rp.ok, rp.failures


def _rejected(c, g_bad):
    r = tr.compare(g_bad, c["g64"], c["g_twin"])
    return (not r.ok), r


@pytest.mark.parametrize("defect", [{"drop_skip": "res3_4"}, {"short_sums": "res3_4.conv2"}, {"short_sums": "conv4_1_2"},
                                    {"own_mask": ("res3_4.conv1", 1e-3)}], ids=lambda d: "%s-%s" % next(iter(d.items())))
def test_compare_rejects_a_defective_backward(defect):
    """One defect at a time in an otherwise exact fp32 twin: the skip gradient of res3_4 lost; BatchNorm's backward sums of a depthwise
    unit without the last four columns of every plane; one unit's mask recomputed from the replay's own sign against a y shifted by 1e-3."""
    c = _standin(1)
    bad, _ = tr.replay(c["sd0"], c["tape"], c["g_hl"], c["g_hs"], torch.float32, defect=defect)
    rejected, r = _rejected(c, bad)
    assert rejected, r.table()
    # ... and what lies downstream of the defect is untouched: the rule names layers, it does not just say "something is off"
    assert not any(s.startswith(("head_4", "conv4_1_5", "head_5", "conv5_6")) for s in r.failures), r.failures


def test_compare_rejects_one_scaled_weight_gradient():
    c = _standin(1)
    for key in ("res2_1.conv1.0.weight", "conv5_3.0.weight", "head_5.weight", "conv0.1.weight"):
        bad = dict(c["g_twin"])
        bad[key] = bad[key] * (1 + 1e-3)
        rejected, r = _rejected(c, bad)
        assert rejected and len(r.failures) == 1 and r.failures[0].startswith(key + ":"), (key, r.failures)
    ok, r = _rejected(c, c["g_twin"])
    assert not ok                                                  # the twin itself passes
    noisy = {k: v.clone() for k, v in c["g_twin"].items()}           # the zero set is held to the twin's noise, not ignored
    noisy[ZERO_SET[3]] = noisy[ZERO_SET[3]] + 10 * r.zero_twin
    assert _rejected(c, noisy)[0]
