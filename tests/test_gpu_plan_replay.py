"""The fp32-storage plans (`precision` f32 and f16x3; fusion 0, 1 and 2) replayed launch by launch on the GPU's own tensors
(tests/replay.py).

For every launch of the plan the input tensor(s) and the output(s) are read back with `model.probe` (the heads: the forward's results); the
inputs go through the float64 evaluation of that ONE launch, and the GPU's output is compared with it element by element, in fp32 ulps at
the size of the terms the element is the sum of.  Nothing accumulates over launches, so a launch is held to tens of ulps where the
head-level rule (test_gpu_parity.py `_check_heads`) allows 3 x torch's own fp32 error 86 layers downstream.  Limit per (precision, launch
kind): 3 x the worst distance of the CPU twin of that precision from the same float64 replay (replay.REFERENCE_F32, measured by
tests/test_cpu_plan_replay.py, whose header table also has the GPU's figures), never more than the launch's a-priori forward-error bound
(replay's "THE CAP"), never taken from the device's own numbers.  Every output must be finite.

Each case asserts the forms it exists for: replay.launch_table restates the launchers' conditions (`mres_small_batch` and its likes)
with the device's own CU count and is held to the engine's op list (`yf_num_launches`, `yf_op_info_ex`) one to one, to the dtype each
kernel is handed (`yf_op_dtype`) and to the dispatches it issues (`yf_op_dispatches`).  A tensor that a launch keeps on chip reports
YF_E_NOPROBE (asserted) and is replayed inside its launch; the scratch tensor of the block-by-block res4 chain has no name, so that op is
replayed as one unit.
"""
import pytest
import torch

from oracle import backbone_oracle as bo
from tests import replay as rp

pytestmark = pytest.mark.gpu
rp.cap_threads()

_GPU_WORST = {}

PARAMS = [(p, f, (H, W, N), w)
          for H, W, N, fusions, precisions in rp.CASES_F32 for f in fusions for p in precisions
          for w in (("random",) if (H, W, N) in rp.RANDOM_ONLY else ("shipped", "random"))]


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
        assert m.split_sums
        out[k] = (m, rp.Net(sd))
    return out


@pytest.mark.parametrize("precision,fusion,case,weights", PARAMS, ids=lambda v: "%dx%d-N%d" % v if isinstance(v, tuple) else str(v))
def test_every_launch_against_its_float64_replay(yf, models, golden, dev, precision, fusion, case, weights):
    m, net = models[weights]
    H, W, N = case
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    x = bo.preprocess(rp.frames_u8(golden, H, W, N))
    xd = x.to(dev)
    table = rp.launch_table(H, W, fusion, precision, N=N, n_cu=n_cu)
    print("\n%s fusion %d %dx%d N=%d %s weights, %d CUs:\n%s" % (precision, fusion, H, W, N, weights, n_cu, rp.forms_text(table)))
    fm = rp.forms(table)
    for name, (kind, disp) in rp.expect(H, W, N, fusion, precision, n_cu).items():     # the forms this case exists for
        assert fm[name][:2] == (kind, disp), (name, fm[name])
    m.fusion, m.precision = fusion, precision
    try:
        ops, tensors = rp.collect(yf, m, table, xd)       # asserts YF_E_NOPROBE for every tensor a launch keeps on chip
        # coverage: the engine's ops and the replay entries are the same list, one to one, with the table's dtypes and dispatches
        assert [o[0] for o in ops] == [L.name for L in table], ([o[0] for o in ops], [L.name for L in table])
        assert [o[1] for o in ops] == [L.dtype for L in table], [(L.name, o[1], L.dtype) for o, L in zip(ops, table) if o[1] != L.dtype]
        assert [o[2] for o in ops] == [L.dispatches for L in table], [(L.name, o[2], L.dispatches) for o, L in zip(ops, table) if o[2] != L.dispatches]
        if fusion == 0:
            assert {o[1] for o in ops} == {rp.DT["f32"]}
    finally:
        m.fusion, m.precision = yf.model.DEFAULT_FUSION, None
    failures = []
    for L in table:
        for n, d, v in rp.replay_and_check(L, net, tensors, tensors, precision):
            w = _GPU_WORST.setdefault((precision, L.kind), [0.0, 0.0, 0.0])
            w[0], w[1], w[2] = max(w[0], d.dist), max(w[1], d.cap_used), max(w[2], d.own)
            print("%-18s %-48s -> %-10s distance %8.3f  (limit %8.2f; share of the cap %.3f; own ulps %.0f)" % (
                L.kind, L.name[:48], n, d.dist, rp.limit(precision, L), d.cap_used, d.own))
            if v:
                failures.append(v)
    assert not failures, "\n".join(failures)


def test_zz_gpu_figures_per_launch_kind():
    """Prints what the header table of tests/test_cpu_plan_replay.py records for the GPU (run with -s)."""
    for k in sorted(_GPU_WORST):
        d, c, o = _GPU_WORST[k]
        print("GPU %-6s %-18s distance %8.2f  twin %8.2f  limit 3 x twin = %8.2f  largest share of the cap used %.3f  (own ulps %.0f)" % (
            k[0], k[1], d, rp.REFERENCE_F32[k], rp.MARGIN * rp.REFERENCE_F32[k], c, o))
