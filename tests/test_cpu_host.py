"""CPU-only tests: weight packer, blob validation, C-ABI exports, host-side API behaviour (no compute without a GPU)."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import yolo_fastest_amd as yf
from yolo_fastest_amd import _lib, packer
from oracle import backbone_oracle as bo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W256 = os.path.join(ROOT, "yolo-fastest-and-embedded-deployment_amd", "assets", "weights", "yolo_fastest_256x320_epoch28.pth")


@pytest.fixture(scope="module")
def sd():
    return bo.load_state_dict(W256)


def test_layer_tables_agree(sd):
    """packer.layer_table (product) and oracle LAYERS (test infra) describe the same 84 conv+BN units, and the
    product's expected key list is exactly the reference checkpoint's key list (strict load, detect.py:91)."""
    t = [l for l in packer.layer_table() if l[1] != packer.KIND_HEAD]
    assert len(t) == len(bo.LAYERS) == 84
    kind = {"c": None, "dw": packer.KIND_DW, "dc": packer.KIND_DECONV}
    for (n, k, ci, co, ks, st, relu), (on, ok, oci, oco, oks, ost, orelu) in zip(t, bo.LAYERS):
        assert (n, ci, co, ks, st, bool(relu)) == (on, oci, oco, oks, ost, orelu)
        if kind[ok] is not None:
            assert k == kind[ok]
    assert packer.expected_keys() == list(sd.keys())


def test_blob_container_and_fold(sd):
    blob = packer.pack_state_dict(sd)
    magic, ver, n, num_out, inch, na, nc, nfl = struct.unpack_from("<8s6IQ", blob, 0)
    assert (magic, ver, n, num_out, inch, na, nc) == (b"YFHIPW01", 1, 86, 24, 1, 3, 3)
    assert len(blob) == 64 + 64 * 86 + 4 * nfl
    u = packer.unpack(blob)
    assert list(u.keys()) == [l[0] for l in packer.layer_table()]
    # fold identity on one unit of each kind: conv(x, w)*s + b' == BN(conv(x, w))
    g = torch.Generator().manual_seed(0)
    for name in ("conv1_2", "conv1_3", "conv1_9", "deconv5_1", "res5_1.conv2"):
        L = u[name]
        ci, co, k = L["cin"], L["cout"], L["k"]
        x = torch.randn(2, ci, 9, 11, generator=g)
        want = bo._unit(sd, name, x)
        w, b = torch.from_numpy(L["w"].copy()), torch.from_numpy(L["b"].copy())
        if L["kind"] == packer.KIND_PW:
            y = F.conv2d(x, w.view(ci, co).t().reshape(co, ci, 1, 1), b)
        elif L["kind"] == packer.KIND_DW:
            y = F.conv2d(x, w.view(k, k, co).permute(2, 0, 1).reshape(co, 1, k, k), b, stride=L["stride"], padding=(k - 1) // 2, groups=co)
        elif L["kind"] == packer.KIND_DENSE:
            y = F.conv2d(x, w.view(k, k, ci, co).permute(3, 2, 0, 1), b, stride=L["stride"], padding=1)
        else:
            y = F.conv_transpose2d(x, w.view(2, 2, ci, co).permute(2, 3, 0, 1), b, stride=2)
        y = F.relu(y) if L["relu"] else y
        assert (y - want).abs().max().item() < 1e-4 * max(1.0, want.abs().max().item()), name
    # heads keep their own bias, no BN
    assert np.allclose(u["head_5"]["b"], sd["head_5.bias"].numpy())
    assert np.allclose(u["head_4"]["w"].reshape(96, 24), sd["head_4.weight"].numpy()[:, :, 0, 0].T)


def test_strict_key_check_like_load_state_dict(sd):
    bad = dict(sd)
    bad.pop("conv0.0.weight")
    with pytest.raises(RuntimeError, match="Missing key"):
        packer.pack_state_dict(bad)
    bad = dict(sd)
    bad["extra.weight"] = torch.zeros(1)
    with pytest.raises(RuntimeError, match="Unexpected key"):
        packer.pack_state_dict(bad)
    m = yf.YoloFastest(yf.config_params["io_params"])
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in sd.items() if k != "head_4.bias"})
    assert str(m.load_state_dict(sd)) == "<All keys matched successfully>"
    assert list(m.state_dict().keys()) == list(sd.keys())
    for k, v in m.state_dict().items():
        assert v.shape == sd[k].shape, k


def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "yolo_fastest_hip.h")).read()
    declared = set(re.findall(r"\b(yf_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) >= 14
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in sorted(declared):
        assert hasattr(L, name), name
    assert declared == set(_lib.EXPORTS)
    assert _lib.lib().yf_abi_version() == 1


def test_create_rejects_bad_arguments_before_touching_the_gpu(sd):
    lib = _lib.lib()
    h = ctypes.c_void_p()
    blob = packer.pack_state_dict(sd)
    buf = ctypes.create_string_buffer(blob, len(blob))
    assert lib.yf_create(buf, len(blob), 250, 320, 4, 0, ctypes.byref(h)) == _lib.YF_E_INVALID  # rows not % 32
    assert b"multiples of 32" in lib.yf_last_error_string()
    assert lib.yf_create(buf, len(blob), 256, 320, 0, 0, ctypes.byref(h)) == _lib.YF_E_INVALID
    bad = bytearray(blob); bad[0:8] = b"NOTABLOB"
    b2 = ctypes.create_string_buffer(bytes(bad), len(bad))
    assert lib.yf_create(b2, len(bad), 256, 320, 4, 0, ctypes.byref(h)) == _lib.YF_E_BLOB
    bad = bytearray(blob); struct.pack_into("<I", bad, 64 + 64 * 5 + 32 + 8, 999)  # layer 5: wrong cout
    b3 = ctypes.create_string_buffer(bytes(bad), len(bad))
    assert lib.yf_create(b3, len(bad), 256, 320, 4, 0, ctypes.byref(h)) == _lib.YF_E_BLOB
    assert b"res1_1.conv2" in lib.yf_last_error_string()
    assert lib.yf_create(buf, 100, 256, 320, 4, 0, ctypes.byref(h)) == _lib.YF_E_BLOB  # truncated
    assert lib.yf_destroy(None) == 0


def test_no_cpu_fallback(sd):
    m = yf.YoloFastest(yf.config_params["io_params"])
    m.load_state_dict(sd)
    with pytest.raises(RuntimeError, match="no CPU path"):          # train mode (the default): training.py, GPU only as well
        m(torch.zeros(1, 1, 256, 320))
    from yolo_fastest_amd import training
    cpu_p = torch.nn.Parameter(torch.zeros(3)); cpu_p.grad = torch.ones(3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        training.Adam([cpu_p]).step()
    m.eval()
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(torch.zeros(1, 1, 256, 320))
    io = yf.io_params_for(256)
    post = yf.YOLO_post_process(io["conf_thre"], io["nms_thre"], 3, 3, io["anchors"], io["input_shape"]).bind(m)
    with pytest.raises(RuntimeError, match="no CPU path"):
        post.detect((torch.zeros(1, 24, 16, 20), torch.zeros(1, 24, 8, 10)))
    with pytest.raises(NotImplementedError):
        yf.YoloFastest(dict(io, input_channel=65))                  # 1 .. 64 input channels are implemented (yf_layers.h MAX_INPUT_CHANNEL)
    six = yf.YoloFastest(dict(io, input_channel=6))                 # more than the fused stem's 4: conv0 becomes a launch of its own
    assert six.conv0[0].weight.shape == (8, 6, 3, 3)
    rgb = yf.YoloFastest(dict(io, input_channel=3, num_cls=5, num_anchors=2)).eval()   # the constructor's three io_params (yolo_fastest.py:72-78)
    assert rgb.conv0[0].weight.shape == (8, 3, 3, 3) and rgb.head_4.weight.shape == (20, 96, 1, 1) and rgb.head_5.bias.shape == (20,)
    with pytest.raises(RuntimeError, match="no CPU path"):
        rgb(torch.zeros(1, 3, 256, 320))
    # the product package never imports the oracle
    import sys
    pkg = os.path.join(ROOT, "yolo-fastest-and-embedded-deployment_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            assert "oracle" not in open(os.path.join(pkg, fn)).read().replace("# oracle", ""), fn


def test_config_mirror():
    io = yf.config_params["io_params"]
    assert io["anchors"][0] == [[10, 13], [16, 30], [33, 23]] and io["input_shape"] == [256, 320, 1]
    assert io["conf_thre"] == 0.5 and io["nms_thre"] == 0.2 and io["class_names"] == ["carrier", "defender", "destroyer"]
    io5 = yf.io_params_for(512)
    assert io5["input_shape"] == [512, 640, 1] and io5["anchors"][0] == [[150, 75], [100, 100], [75, 150]]
    tp = yf.config_params["train_params"]                      # _config.py:38-50
    assert (tp["total_epochs"], tp["batch_size"], tp["lr0"], tp["IOU_loss_thre"], tp["IOU_val_thre"]) == (30, 16, 0.001, 0.5, 0.5)
    from yolo_fastest_amd import training                      # train.py:87-88
    assert training.cosine_factor(0, 30) == 1.0 and abs(training.cosine_factor(30, 30) - 0.2) < 1e-12
    assert abs(training.cosine_factor(15, 30) - 0.6) < 1e-12


W512 = os.path.join(ROOT, "yolo-fastest-and-embedded-deployment_amd", "assets", "weights", "yolo_fastest_512x640_epoch27.pth")
SHIPPED = {"256x320": W256, "512x640": W512}     # models/{ncnn,onnx}/<size>/ of the reference, copied (data) to tests/golden/{ncnn,onnx}/


@pytest.mark.parametrize("size", ["256x320", "512x640"])
def test_ncnn_model_files_give_the_same_blob(size):
    """the reference's shipped ncnn .param/.bin (BN already folded by its converter; both sizes, models/ncnn/256x320 and
    /512x640) packs to the same blob as the .pth of that size folded here -- to fp32 rounding of two different fold orders."""
    sd = bo.load_state_dict(SHIPPED[size])
    pth = packer.unpack(packer.pack_state_dict(sd))
    ncnn = packer.unpack(packer.pack_ncnn(os.path.join(ROOT, "tests", "golden", "ncnn", f"yolo_fastest_{size}.param"),
                                          os.path.join(ROOT, "tests", "golden", "ncnn", f"yolo_fastest_{size}.bin")))
    assert list(pth) == list(ncnn)
    for k in pth:
        for f in ("kind", "cin", "cout", "k", "stride", "relu"):
            assert pth[k][f] == ncnn[k][f], (k, f)
        assert np.abs(pth[k]["w"] - ncnn[k]["w"]).max() < 5e-6, k
        assert np.abs(pth[k]["b"] - ncnn[k]["b"]).max() < 5e-6, k
    with pytest.raises(ValueError):
        packer.read_ncnn(W256, W256)  # not a .param file


def test_host_f32_to_f16_rounding_is_ieee_rne():
    """The fp16 weight streams are rounded on the host (yf_mfma_kernels.hip f32_to_f16_bits): must equal IEEE
    round-to-nearest-even = numpy's float16 cast, including subnormals, ties, overflow to inf, signed zero, nan."""
    from yolo_fastest_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(0)
    bits = rng.integers(0, 2 ** 32, 20000, dtype=np.uint64).astype(np.uint32)
    vals = np.concatenate([
        bits.view(np.float32),
        (rng.standard_normal(5000) * 10.0 ** rng.integers(-9, 6, 5000)).astype(np.float32),
        np.array([0.0, -0.0, 1.0, -1.0, 65504.0, 65519.9, 65520.0, 1e9, -1e9, np.inf, -np.inf, 2.0 ** -24, 2.0 ** -25,
                  2.0 ** -25 * 1.0000001, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11,
                  1.0 + 2.0 ** -11 + 2.0 ** -20, 6.1e-5, 5.96e-8, 2.98e-8, 2.99e-8], np.float32)])
    with np.errstate(over="ignore", invalid="ignore"):
        want = vals.astype(np.float16).view(np.uint16)
    for v, w in zip(vals.tolist(), want.tolist()):
        got = L.yf_f32_to_f16_bits(v)
        if v != v:
            assert (got & 0x7C00) == 0x7C00 and (got & 0x3FF) != 0
        else:
            assert got == w, (v, hex(got), hex(w))


def test_validation_bookkeeping_matches_the_oracle(golden):
    """Host logic of yolo_fastest_amd.validation.Validation (matching + AP arithmetic, validate.py:47-119) against the
    oracle's literal restatement: on the reference's stored NMS output, and on random match lists (ties, repeated recalls)."""
    import logging
    from oracle import val_oracle as vo
    from yolo_fastest_amd import validation as V
    g = golden("golden_map_256")
    params = {"train_params": {"batch_size": 4, "IOU_val_thre": 0.5},
              "io_params": {"input_shape": (256, 320, 1), "num_cls": 3, "class_names": ["carrier", "defender", "destroyer"],
                            "conf_thre": 0.5, "nms_thre": 0.2}}
    frames = [(np.zeros((2, 2, 1), np.float32), np.zeros((64, 6), np.float32))] * 4   # the loader is not used here
    val = V.Validation(params, logging.getLogger("t"), frames, "cpu", None)
    rec = val._recover_targets(torch.from_numpy(g["targets"]))
    assert torch.equal(rec, vo.recover_targets(torch.from_numpy(g["targets"]), (256, 320, 1)))
    for f in range(len(g["count"])):
        val._match_image(torch.from_numpy(g["det"][f, :g["count"][f]]) if g["count"][f] else None, rec[f])
    for c in range(3):
        val.match_list[c].sort(key=lambda x: x[0], reverse=True)
    aps = [val._calculate_AP(c) for c in range(3)]
    assert [float(a) for a in aps] == g["AP"].tolist()
    assert val.target_num.tolist() == g["target_num"].tolist()
    rng = np.random.default_rng(0)
    for trial in range(50):
        n = int(rng.integers(0, 40))
        val.clear()
        val.match_list[0] = [("k", bool(rng.integers(0, 2))) for _ in range(n)]
        tp = sum(m[1] for m in val.match_list[0])
        val.target_num[0] = tp + int(rng.integers(0, 5)) if n else int(rng.integers(0, 3))
        want = vo.calculate_ap(val.match_list[0], val.target_num[0]) if n else 0
        got = float(val._calculate_AP(0))
        assert got == float(want) or (got != got and float(want) != float(want)), (trial, n)   # 0 targets and 0 TP: nan in both


@pytest.mark.parametrize("size", ["256x320", "512x640"])
def test_onnx_export_gives_the_same_state_dict(size):
    """the reference's shipped ONNX exports (models/onnx/256x320 and /512x640, copied to tests/golden/onnx) read with the
    built-in protobuf reader are the shipped .pth of that size, key for key and bit for bit, hence the same blob."""
    from yolo_fastest_amd import packer
    sd = bo.load_state_dict(SHIPPED[size])
    got = packer.read_onnx(os.path.join(ROOT, "tests", "golden", "onnx", f"yolo_fastest_{size}.onnx"))
    assert set(got) == set(sd)
    for k, v in sd.items():
        if v.is_floating_point():
            assert torch.equal(v.float().cpu(), got[k]), k
    assert packer.pack_state_dict(got) == packer.pack_state_dict(sd)
    # structure checks: a truncated graph is refused
    with pytest.raises(Exception):
        packer.read_onnx(os.path.join(ROOT, "tests", "golden", "ncnn", "yolo_fastest_256x320.param"))


def _run_bench(args, env_extra=None, timeout=300):
    import subprocess, sys
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True, timeout=timeout)


def test_bench_gpus_n_never_degrades_silently():
    """bench.py's launch contract (VERDICT r1 / ADVICE): `--gpus N` with N > visible GPUs exits non-zero with a message and prints no
    JSON line; a launcher whose WORLD_SIZE disagrees with --gpus is refused the same way.  (Here no GPU is visible at all.)"""
    if torch.cuda.device_count() >= 8:
        pytest.skip("host has 8 GPUs: the refusal path is not reachable")
    r = _run_bench(["--gpus", "8", "--steps", "1", "--warmup", "0"])
    assert r.returncode != 0 and "GPU(s) are visible" in r.stderr and '"n_gpus"' not in r.stdout, (r.returncode, r.stderr[-300:])
    r = _run_bench(["--gpus", "4", "--steps", "1", "--warmup", "0"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE=2" in r.stderr + r.stdout and '"n_gpus"' not in r.stdout
    r = _run_bench(["--gpus", "1", "--steps", "1", "--warmup", "0"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and '"n_gpus"' not in r.stdout


def test_bench_dump_ops_needs_full():
    """The launch list of --dump-ops comes from the per-launch timing, which only a --full run does: a plain run asking for it is
    refused before it touches the GPU instead of finishing without the file."""
    r = _run_bench(["--gpus", "1", "--steps", "1", "--warmup", "0", "--dump-ops", os.devnull])
    assert r.returncode != 0 and "--dump-ops needs --full" in r.stderr and '"n_gpus"' not in r.stdout, (r.returncode, r.stderr[-300:])


def test_bench_roofline_arithmetic():
    """The physical-roof arithmetic of bench.launch_roofline: fp32 prices all flops against the shared 157.3 TF issue rate, fp16
    prices MFMA flops against the fp16 MFMA peak (never against the fp32 peak: no fraction above 1 from a unit mix-up), and a
    launch whose counter bytes per second exceed half the streaming rate is reported HBM-bound."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec); spec.loader.exec_module(b)
    o = dict(ms=0.1, flops=15.73e9, mfma_flops=12e9, valu_flops=3.73e9)
    r = b.launch_roofline(o, "f32", None)
    assert r["bound"] == "mfma" and abs(r["compute_frac"] - 1.0) < 1e-9 and r["hbm_frac"] is None
    r = b.launch_roofline(o, "f32", 0.1e-3 * 5.0e12)          # 5 TB/s measured -> HBM-bound, frac vs the 8 TB/s spec
    assert r["bound"] == "hbm" and abs(r["frac"] - 5.0 / 8.0) < 1e-9
    r = b.launch_roofline(o, "f16", 0.1e-3 * 1.0e12)
    assert r["bound"] in ("mfma", "valu") and r["compute_frac"] <= 1.0
    assert abs(r["compute_frac"] - max(12e9 / 2.5e15, 3.73e9 / 157.3e12) / 1e-4) < 1e-9
    assert abs(r["issued_frac"] - r["compute_frac"]) < 1e-12            # single fp16 operands: issued == useful
    # split operands (f16x3): three MFMAs per product are ISSUED; `frac` / `achieved` count the useful third, `issued_frac` the rest
    o3 = dict(ms=0.1, flops=101e9, mfma_flops=100e9, valu_flops=1e9)
    r1, r3 = b.launch_roofline(o3, "f16", None), b.launch_roofline(o3, "f16x3", None)
    assert r3["on_mfma"] and abs(r3["compute_frac"] - 100e9 / 2.5e15 / 1e-4) < 1e-9 and abs(r3["frac"] - r1["frac"]) < 1e-12
    assert abs(r3["issued_frac"] - 3 * r3["compute_frac"]) < 1e-9 and abs(r3["achieved_tf"] - 100e9 / 1e-4 / 1e12) < 1e-6
    # the issued work (not the useful third) decides which pipe is the busier one
    o4 = dict(ms=0.1, flops=30e9, mfma_flops=20e9, valu_flops=2e9)       # mfma 8 us useful / 24 us issued, valu 12.7 us
    assert not b.launch_roofline(o4, "f16", None)["on_mfma"] and b.launch_roofline(o4, "f16x3", None)["on_mfma"]
    assert len(b.source_hash()) == 16


def test_bench_dump_outputs(tmp_path):
    """bench.dump_outputs (--dump-outputs): the records and heads of a step as DIR/<name>.npy in float32 / float64, integer records exact,
    the slots past a frame's count zeroed (never written by the post-process), and over the byte budget a seeded sample of frames that
    is the same from call to call; an array covering only the first frames (N > 1: rank 0's heads) keeps the sampled frames it has."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec); spec.loader.exec_module(b)
    rng = np.random.default_rng(1)
    n, kmax = 40, 8
    counts = np.array([3, 0, 9, -2] + [5] * (n - 4), np.int32)        # 9 > kmax: overflow, the first kmax stored; -2: no records
    res = dict(counts=counts, boxes=rng.integers(-2**31, 2**31, (n, kmax, 4), dtype=np.int32),
               scores=rng.standard_normal((n, kmax, 2)).astype(np.float32), cls=rng.integers(0, 3, (n, kmax), dtype=np.int32),
               src=rng.integers(0, 2**31, (n, kmax), dtype=np.int32), head_large=rng.standard_normal((n, 24, 4, 5)).astype(np.float32),
               head_small=rng.standard_normal((n, 24, 2, 3)).astype(np.float32))
    names = b.dump_outputs(str(tmp_path / "all"), res)
    assert names == sorted(res)
    got = {k: np.load(tmp_path / "all" / (k + ".npy")) for k in names}
    assert all(got[k].dtype == (np.float32 if k in ("scores", "head_large", "head_small") else np.float64) for k in names)
    valid = np.arange(kmax)[None, :] < np.clip(counts, 0, kmax)[:, None]
    assert valid[2].all() and not valid[3].any()
    for k in ("boxes", "scores", "cls", "src"):
        assert np.array_equal(got[k][valid], res[k][valid].astype(got[k].dtype)) and not got[k][~valid].any(), k
    assert np.array_equal(got["counts"], counts) and np.array_equal(got["head_large"], res["head_large"])
    # over the budget: a sample of frames, in frame order, every file within it, the same frames every time
    budget = 16 << 10
    for d in ("s1", "s2"):
        names = b.dump_outputs(str(tmp_path / d), dict(res, head_small=res["head_small"][:10]), budget=budget)
        assert "frames" in names and sum(os.path.getsize(tmp_path / d / (k + ".npy")) for k in names) <= budget
    fr = np.load(tmp_path / "s1" / "frames.npy")
    assert 1 <= len(fr) < n and np.all(np.diff(fr) > 0) and np.array_equal(fr, np.load(tmp_path / "s2" / "frames.npy"))
    for k in names:
        a = np.load(tmp_path / "s1" / (k + ".npy"))
        assert np.array_equal(a, np.load(tmp_path / "s2" / (k + ".npy"))), k
    fr = fr.astype(int)
    assert np.array_equal(np.load(tmp_path / "s1" / "head_large.npy"), res["head_large"][fr])
    assert np.array_equal(np.load(tmp_path / "s1" / "head_small.npy"), res["head_small"][fr[fr < 10]])
    assert np.array_equal(np.load(tmp_path / "s1" / "counts.npy"), counts[fr])
    with pytest.raises(ValueError):
        b.dump_outputs(str(tmp_path / "bad"), dict(res, head_large=np.zeros((n + 1, 2), np.float32)))


CLASS_RGB ={0: (205, 90, 106), 1: (20, 97, 199), 2: (105, 128, 112)}   # detect.py:105 colours are BGR (cv2); these are what a viewer sees


def test_reference_result_images_carry_the_golden_boxes(golden):
    """SURVEY.md 8(f).3 pin: tests/golden/golden_results.npz holds pixels sampled from the reference's OWN result images
    (test_result/*/<laptop cpu>_test_result/result_*.jpg) at the edge midpoints of the boxes the goldens predict: every one
    has its class colour there (JPEG tolerance), for all 20 frames x both checkpoints; and the logged has-target flags are the
    goldens' (make_golden.py main_results asserts that when it builds the file)."""
    r = golden("golden_results")
    for res in (256, 512):
        g = golden(f"golden_{res}")
        assert [str(n) for n in r[f"names_{res}"]] == [str(n) for n in g["names"]]
        assert r[f"finished_{res}"].tolist() == [bool(c) for c in g["adj_count"]]
        nbox = 0
        for f in range(20):
            for k in range(int(g["adj_count"][f])):
                want = np.array(CLASS_RGB[int(g["adj_cls"][f, k])], np.int32)
                for j in range(4):
                    assert np.abs(r[f"edge_rgb_{res}"][f, k, j].astype(np.int32) - want).max() <= 40, (res, f, k, j)
                nbox += 1
        assert nbox >= 25
    assert not r["finished_512"][14] and r["finished_256"].all()


def test_plot_one_box_geometry():
    """plot.plot_one_box (general.py:56-67 without cv2): a frame of width `line_thickness` centred on the box edges in the class
    colour (as a viewer sees the reference's BGR colour), a filled label box above the top-left corner, nothing elsewhere."""
    from yolo_fastest_amd.plot import plot_one_box
    img = np.zeros((120, 200, 3), np.uint8)
    out = plot_one_box([40, 50, 120, 90], img, color=[106, 90, 205], label="carrier 0.63", line_thickness=3)
    assert out is img
    rgb = (205, 90, 106)
    for (x, y) in ((80, 50), (80, 90), (40, 70), (120, 70), (80, 49), (80, 51), (39, 70), (121, 70)):
        assert tuple(img[y, x]) == rgb, (x, y, img[y, x])
    for (x, y) in ((80, 70), (80, 47 + 60), (37, 70), (123, 70), (150, 20)):
        assert tuple(img[y, x]) == (0, 0, 0), (x, y)
    lab = img[50 - 3 - 13:50 - 1, 40:60].astype(np.int32)     # label box: from c1 upwards, th = round(22 * 3/5) = 13
    lo, hi = np.minimum(rgb, (255, 255, 225)), np.maximum(rgb, (255, 255, 225))   # anti-aliased text: box colour .. text colour
    assert ((lab >= lo - 1) & (lab <= hi + 1)).all() and tuple(lab[0, 0]) == rgb
    assert (img.astype(np.int32).sum(-1) > 600).sum() > 20     # some (near-)text-coloured pixels: [225, 255, 255] BGR
    # no label, default thickness round(0.002 * (h + w) / 2) + 1 = 1
    img2 = np.zeros((120, 200, 3), np.uint8)
    plot_one_box([10, 10, 30, 30], img2, color=[0, 0, 255])
    assert tuple(img2[10, 20]) == (255, 0, 0) and tuple(img2[11, 20]) == (0, 0, 0)


def _fake_sysfs(root, gpu_numa, node_cpus):
    """A sysfs tree with one KFD CPU node, len(gpu_numa) GPU nodes (numa_node as given; None: the PCI file is missing) and the NUMA cpulists."""
    nodes = os.path.join(root, "class/kfd/kfd/topology/nodes")
    os.makedirs(os.path.join(nodes, "0"))
    open(os.path.join(nodes, "0", "properties"), "w").write("cpu_cores_count 64\nsimd_count 0\n")
    for i, numa in enumerate(gpu_numa):
        os.makedirs(os.path.join(nodes, str(i + 1)))
        loc = ((0x10 + i) << 8)          # bus 0x10 + i, device 0, function 0
        open(os.path.join(nodes, str(i + 1), "properties"), "w").write(f"simd_count 1024\nlocation_id {loc}\ndomain 0\n")
        if numa is not None:
            d = os.path.join(root, "bus/pci/devices/0000:%02x:00.0" % (0x10 + i))
            os.makedirs(d)
            open(os.path.join(d, "numa_node"), "w").write(f"{numa}\n")
    for node, cl in node_cpus.items():
        d = os.path.join(root, f"devices/system/node/node{node}")
        os.makedirs(d)
        open(os.path.join(d, "cpulist"), "w").write(cl + "\n")


def test_rank_cpu_plan_uses_one_scheme_for_all_ranks(tmp_path):
    """bench.plan_rank_cpus decides the slicing scheme ONCE for all local ranks -- NUMA shares only if every rank's GPU resolves,
    else contiguous slices for everyone -- and the slices are disjoint either way (a faked sysfs tree; no GPU, no real topology)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec); spec.loader.exec_module(b)
    allowed = list(range(64))
    # all four GPUs resolve: two per NUMA node, each rank half of its node
    t1 = str(tmp_path / "a"); _fake_sysfs(t1, [0, 0, 1, 1], {0: "0-15,32-47", 1: "16-31,48-63"})
    sl, how = b.plan_rank_cpus(4, allowed, t1)
    assert "NUMA" in how and sl[0] == list(range(0, 16)) and sl[1] == list(range(32, 48)) and sl[2] == list(range(16, 32)) and sl[3] == list(range(48, 64))
    # one GPU reports numa_node -1: EVERY rank falls back to contiguous slices (no mixing of the two schemes)
    t2 = str(tmp_path / "b"); _fake_sysfs(t2, [0, 0, -1, 1], {0: "0-15,32-47", 1: "16-31,48-63"})
    sl, how = b.plan_rank_cpus(4, allowed, t2)
    assert "contiguous" in how and sl == [list(range(16 * r, 16 * r + 16)) for r in range(4)]
    # a missing PCI entry (OSError) and a node with fewer than two CPUs per rank: the same fallback
    t3 = str(tmp_path / "c"); _fake_sysfs(t3, [0, None, 1, 1], {0: "0-31", 1: "32-63"})
    assert "contiguous" in b.plan_rank_cpus(4, allowed, t3)[1]
    t4 = str(tmp_path / "d"); _fake_sysfs(t4, [0, 0, 0, 0], {0: "0-5", 1: "6-63"})
    assert "contiguous" in b.plan_rank_cpus(4, allowed, t4)[1]
    # HIP_VISIBLE_DEVICES narrows and reorders the GPU list before ranks are mapped
    sl, how = b.plan_rank_cpus(2, allowed, t1, visible="3,0")
    assert "NUMA" in how and sl[0] == list(range(16, 32)) + list(range(48, 64)) and sl[1] == list(range(0, 16)) + list(range(32, 48))
    # no sysfs at all
    sl, how = b.plan_rank_cpus(8, allowed, str(tmp_path / "none"))
    assert "contiguous" in how and sum(len(x) for x in sl) == 64 and len({c for x in sl for c in x}) == 64


def test_bench_pins_each_rank_to_its_own_cpu_slice():
    """bench.py pins a rank to a slice of the host's CPUs before its first GPU call.  In a child process per rank (the
    mask is inherited by whatever the process starts afterwards): the slices of four ranks are disjoint, non-empty subsets of the allowed
    set; one rank alone is left unpinned."""
    import json
    import subprocess
    import sys
    code = ("import json, os, sys; sys.path.insert(0, %r); sys.argv = ['bench.py']; import bench\n"
            "before = sorted(os.sched_getaffinity(0)); info = bench.pin_rank_to_cpus(int(sys.argv_rank), int(sys.argv_world))\n"
            "print(json.dumps({'before': before, 'after': sorted(os.sched_getaffinity(0)), 'info': info}))\n") % ROOT
    allowed = sorted(os.sched_getaffinity(0))
    if len(allowed) < 8:
        pytest.skip("needs at least 8 allowed CPUs for four ranks")
    seen = []
    for rank in range(4):
        r = subprocess.run([sys.executable, "-c", code.replace("sys.argv_rank", "'%d'" % rank).replace("sys.argv_world", "'4'")],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        out = json.loads(r.stdout.strip().splitlines()[-1])
        assert out["before"] == allowed and out["info"] is not None and out["info"]["cpus"] == len(out["after"]) >= 2
        assert set(out["after"]) <= set(allowed)
        seen.append(set(out["after"]))
    assert all(not (a & b) for i, a in enumerate(seen) for b in seen[i + 1:])
    r = subprocess.run([sys.executable, "-c", code.replace("sys.argv_rank", "'0'").replace("sys.argv_world", "'1'")], capture_output=True, text=True, timeout=300)
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["info"] is None and out["after"] == allowed
