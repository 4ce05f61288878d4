"""The io-dependent launches -- the stem, the separate conv0 of more than four input planes (and the block behind it), the two head
launches -- at other io_params than the shipped ones, replayed on the GPU's own tensors in every tile form the launchers have for them
(tests/replay.py IO_CASES; the CPU side, the twin's figures and the device's are in tests/test_cpu_io_replay.py).

tests/test_gpu_io_params.py reaches these launches at 2 frames of 256x320 and judges them at the heads, 86 layers downstream.  Here each
launch is evaluated in float64 from the input tensor(s) the device produced (`model.probe`) and compared element by element:
  fp32 storage   replay.replay_and_check under replay.limit: 3 x the twin's distance of that (precision, kind), never above the launch's cap;
  fp16 storage   replay.verdict / replay.limits (SHARE_CAP, ULP_CAP), and the share of fp32 logits outside F32_RTOL of the range.
The twin's figures are those of the shipped shape (REFERENCE_F32, REFERENCE_F16, F32_REFERENCE_F16) except where tests/test_cpu_io_replay.py
found a configuration to exceed them: replay.IO_REFERENCE_*.  Never the device's own numbers.

The table (`replay.launch_table(..., num_out, input_channel, head_forms=True)`) is held to the engine's op list, dtypes and dispatch counts
one to one, and each case asserts the forms it exists for with the device's own CU count: the `many` case FAILS if the launcher does not take
16x20 tiles there.
"""
import pytest
import torch

from oracle import backbone_oracle as bo
from tests import io_cfg
from tests import replay as rp

pytestmark = pytest.mark.gpu
rp.cap_threads()

_GPU_WORST = {}
_MODELS = {}


@pytest.fixture(scope="module")
def yf():
    import yolo_fastest_amd
    return yolo_fastest_amd


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _model(yf, dev, golden, tag):
    import os
    assert "YF_DEEP_MASK" not in os.environ, "the developer switch changes the level-2 plan this test models"
    if tag not in _MODELS:
        C, Cin, A = io_cfg.CONFIG[tag]
        sd = io_cfg.state_dict_for(tag, int(golden("golden_io")[tag + "_seed"]))
        m = yf.YoloFastest(io_cfg.io_for(tag)).to(dev).eval()
        m.load_state_dict({k: v.to(dev) for k, v in sd.items()})   # strict
        assert m.split_sums and m.num_out == A * (5 + C)
        _MODELS[tag] = (m, rp.Net(sd, A * (5 + C), Cin))
    return _MODELS[tag]


@pytest.mark.parametrize("case,H,W,N,tag,precision,fusion", rp.io_params_list(), ids=str)
def test_io_dependent_launches_against_their_float64_replay(yf, dev, golden, case, H, W, N, tag, precision, fusion):
    m, net = _model(yf, dev, golden, tag)
    C, Cin, A = io_cfg.CONFIG[tag]
    num_out = A * (5 + C)
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    N = rp.io_batch(N, n_cu)
    xd = bo.preprocess(io_cfg.io_inputs(tag, Cin, N, H, W), Cin).to(dev)
    table = rp.launch_table(H, W, fusion, precision, N=N, n_cu=n_cu, num_out=num_out, input_channel=Cin, head_forms=True)
    launches = rp.io_launches(table)
    print("\n%s %s %s fusion %d %dx%d N=%d, %d CUs:\n%s" % (case, tag, precision, fusion, H, W, N, n_cu, rp.forms_text(launches)))
    fm = rp.forms(table)
    want = rp.io_expect(case, H, W, N, fusion, precision, num_out, Cin)
    assert sorted(want) == sorted(L.name for L in launches)
    for name, (kind, disp, form) in want.items():
        assert fm[name][:2] == (kind, disp) and (not form or fm[name][2] == form), (name, fm[name], want[name])
    if case == "many":
        assert "16x20" in fm[rp.HEAD_L][2] and "8x10" in fm[rp.HEAD_S][2], fm
    m.fusion, m.precision = fusion, precision
    try:
        ops, tensors = rp.collect(yf, m, table, xd, launches)   # the op list is held to the whole table; YF_E_NOPROBE for what a launch keeps on chip
        assert [o[1] for o in ops] == [L.dtype for L in table], [(L.name, o[1], L.dtype) for o, L in zip(ops, table) if o[1] != L.dtype]
        assert [o[2] for o in ops] == [L.dispatches for L in table], [(L.name, o[2], L.dispatches) for o, L in zip(ops, table) if o[2] != L.dispatches]
    finally:
        m.fusion, m.precision = yf.model.DEFAULT_FUSION, None
        m.refresh()                                              # 8 models x 3 sizes x 3 dtypes of engines are not kept
    r32, r16, f16 = rp.io_references(tag)
    failures = []
    for L in launches:
        hm = L.form if L.kind.startswith("mdw") else ""
        for res in rp.replay_and_check(L, net, tensors, tensors, precision, r16 if precision == "f16" else r32, f16):
            if precision == "f16":
                n, c, share, v = res
                if not L.fp32_out:
                    assert torch.equal(tensors[n], tensors[n].half().float()), n
                w = _GPU_WORST.setdefault((precision, L.kind, hm), [0.0, 0.0, 0.0])
                w[0], w[1], w[2] = max(w[0], share), max(w[1], c.dist), max(w[2], c.share if L.fp32_out else 0.0)
                print("%-12s %-14s %-44s -> %-10s share %.4f %%  distance %.3f%s" % (
                    L.kind, hm, L.name[:44], n, 100 * share, c.dist, "; outside the fp32 criterion %.3f %%" % (100 * c.share) if L.fp32_out else ""))
            else:
                n, d, v = res
                w = _GPU_WORST.setdefault((precision, L.kind, hm), [0.0, 0.0, 0.0])
                w[0], w[1] = max(w[0], d.dist), max(w[1], d.cap_used)
                print("%-12s %-14s %-44s -> %-10s distance %8.3f  (limit %8.2f; share of the cap %.3f)" % (
                    L.kind, hm, L.name[:44], n, d.dist, rp.limit(precision, L, r32), d.cap_used))
            if v:
                failures.append(v)
    assert not failures, "\n".join(failures)


def test_zz_gpu_figures_per_kind_head_mode_and_tile():
    """Prints what the header table of tests/test_cpu_io_replay.py records for the GPU (run with -s)."""
    for k in sorted(_GPU_WORST):
        a, b, c = _GPU_WORST[k]
        if k[0] == "f16":
            print("GPU %-6s %-12s %-14s share %.4f %%  distance %.3f  outside the fp32 criterion %.3f %%" % (k + (100 * a, b, 100 * c)))
        else:
            print("GPU %-6s %-12s %-14s distance %8.2f  largest share of the cap used %.3f" % (k + (a, b)))
