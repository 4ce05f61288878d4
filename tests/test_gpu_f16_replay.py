"""The fp16-storage plan (`dtype f16`) replayed launch by launch on the GPU's own tensors (tests/replay.py, `precision` "f16").

For every launch of the plan the input tensor(s) and the output(s) are read back with `model.probe` (the heads: the forward's results);
the inputs -- the GPU's own fp16 values, exactly representable -- go through the float64 replay of that ONE launch, which rounds where the
kernel rounds, and the GPU's output is compared with it element by element.  No rounding accumulates over launches, so the criteria are
fractions of a per cent of a launch's elements and one or two fp16 ulps, where the head-level fp16 bounds are hundreds of ulps of an
interior tensor.  Criteria per launch kind: replay.limits -- the margin (3) times the share of elements by which the float32 CPU twin of
the same launch differs from the float64 replay, never more than 2 %; the twin's largest distance + 1 ulp, never more than 8.  The twin's
figures and the GPU's are in the header table of tests/test_cpu_f16_replay.py.

Fusion levels 1 and 2: level 0 (one launch per layer) has no fp16-storage form, the engine refuses it (asserted below).  With YF_DEEP_MASK
unset level 2's un-rounded on-chip tensors (res5_5 in front of conv5_2, conv5_4 inside the small head) are part of the model.  A tensor that a
launch keeps on chip reports YF_E_NOPROBE (asserted); it is replayed inside its launch.  The table is held to the engine's own list of
launches (`yf_num_launches`, `yf_op_info_ex`): every op is covered by exactly one replay entry.
"""
import pytest
import torch

from oracle import backbone_oracle as bo
from tests import replay as rp

pytestmark = pytest.mark.gpu
rp.cap_threads()

_GPU_WORST = {}


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
    import os
    assert "YF_DEEP_MASK" not in os.environ, "the developer switch changes the level-2 plan this test models"
    out = {}
    for k, load in rp.state_dicts().items():
        sd = load()
        m = yf.YoloFastest(yf.io_params_for(256)).to(dev).eval()
        m.load_state_dict(sd)
        m.storage_dtype = torch.float16
        out[k] = (m, rp.Net(sd))
    return out


@pytest.mark.parametrize("fusion", [1, 2])
@pytest.mark.parametrize("case", rp.CASES_F16, ids=lambda c: "%dx%d-N%d" % c)
@pytest.mark.parametrize("weights", ["shipped", "random"])
def test_every_launch_against_its_float64_replay(yf, models, golden, dev, weights, case, fusion):
    m, net = models[weights]
    H, W, N = case
    x = bo.preprocess(rp.frames_u8(golden, H, W, N))
    xd = x.to(dev)
    table = rp.launch_table(H, W, fusion, "f16", N=N)
    m.fusion = fusion
    try:
        ops, tensors = rp.collect(yf, m, table, xd)       # asserts YF_E_NOPROBE for every tensor a launch keeps on chip
        # coverage: the engine's ops and the replay entries are the same list, one to one, and every kernel is handed the fp16 dtype
        assert [o[0] for o in ops] == [L.name for L in table], ([o[0] for o in ops], [L.name for L in table])
        assert {o[1] for o in ops} == {1} == {L.dtype for L in table}, ops
    finally:
        m.fusion = yf.model.DEFAULT_FUSION
    for n, t in tensors.items():
        if n != "input" and not n.startswith("head_"):
            assert torch.equal(t, t.half().float()), n       # fp16 storage: the probes are fp16 values
    failures = []
    for L in table:
        for n, c, share, v in rp.replay_and_check(L, net, tensors, tensors, "f16", rp.REFERENCE_F16):
            w = _GPU_WORST.setdefault(L.kind, [0.0, 0.0, 0.0, 0.0])
            w[0], w[1], w[2], w[3] = max(w[0], share), max(w[1], c.dist), max(w[2], c.ulps), max(w[3], c.share if L.fp32_out else 0.0)
            print("%-16s %-48s -> %-10s share %.4f %%  distance %.3f  (own ulps %.0f%s)" % (
                L.kind, L.name[:48], n, 100 * share, c.dist, c.ulps, "; outside the fp32 criterion %.3f %%" % (100 * c.share) if L.fp32_out else ""))
            if v:
                failures.append(v)
    assert not failures, "\n".join(failures)


def test_level_0_has_no_fp16_storage_form(yf, models, golden, dev):
    """Why the replay covers fusion levels 1 and 2 only: the per-layer plan is refused with fp16 storage."""
    m, _ = models["shipped"]
    xd = bo.preprocess(rp.frames_u8(golden, 96, 160, 2)).to(dev)
    m.fusion = 0
    try:
        with pytest.raises(yf._lib.YFError, match="fused plan"):
            m(xd)
    finally:
        m.fusion = yf.model.DEFAULT_FUSION


def test_zz_gpu_figures_per_launch_kind():
    """Prints what the header table of tests/test_cpu_f16_replay.py records for the GPU (run with -s)."""
    for k in sorted(_GPU_WORST):
        s, d, u, f = _GPU_WORST[k]
        print("GPU %-16s share %.4f %%  distance %.3f  (own ulps %.0f; outside the fp32 criterion %.3f %%)  limits %s" % (
            k, 100 * s, d, u, 100 * f, rp.limits(k, rp.REFERENCE_F16)))
