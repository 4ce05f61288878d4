"""Host side of `Validation(..., match="device")` (validation.py): the sort-key formatter `_conf_keys` against `str(tensor)` itself, the
constructor's refusal, and yf_val_match's argument checks, which return before anything touches a GPU."""
import ctypes
import logging

import numpy as np
import pytest
import torch

from yolo_fastest_amd import _lib, validation as V

F32 = np.float32
T1E4 = F32(1e-4)
PLANTED = [F32(0.0), F32(1.0), F32(1.0) - F32(2.0 ** -24), F32(0.99995), F32(0.999949), F32(0.5), T1E4, np.nextafter(T1E4, F32(0)),
           np.nextafter(T1E4, F32(1)), F32(2.0 ** -149)]


def _str_keys(values):
    return [str(torch.tensor(float(v), dtype=torch.float32)) for v in values]


@pytest.fixture()
def fallbacks(monkeypatch):
    """the tensors that reach `_key_fallback` (str() of one 0-dim tensor)"""
    seen = []

    def counting(t):
        seen.append(float(t))
        return str(t)
    monkeypatch.setattr(V, "_key_fallback", counting)
    return seen


def test_keys_equal_str_of_the_tensor(golden, fallbacks):
    g = golden("golden_map_256")
    conf = np.concatenate([g["det"][f, :g["count"][f], 4] for f in range(len(g["count"]))]).astype(np.float32)
    assert len(conf) == int(g["count"].sum()) > 30 and conf.min() >= 0.5
    uniform = np.random.default_rng(0).uniform(0, 1, 20000).astype(np.float32)
    uniform = uniform[uniform < 1]
    planted = np.array(PLANTED, np.float32)
    assert planted[2] < 1 and planted[7] < planted[6] < planted[8] and planted[9] > 0
    for name, vals in (("golden", conf), ("uniform", uniform), ("planted", planted)):
        got = V._conf_keys(torch.from_numpy(vals))
        want = _str_keys(vals)
        bad = [(float(v), a, b) for v, a, b in zip(vals, got, want) if a != b]
        assert not bad, (name, len(bad), bad[:5])
    assert fallbacks == []                                   # all of it through the fast form
    assert V._conf_keys(torch.from_numpy(planted))[:2] == ["tensor(0.)", "tensor(1.)"]


def test_str_fallback_for_what_the_fast_form_does_not_cover(fallbacks):
    odd = torch.tensor([float("nan"), 2.0, -0.0, -0.25, float("inf")], dtype=torch.float32)
    assert V._conf_keys(odd) == [str(v) for v in odd] == ["tensor(nan)", "tensor(2.)", "tensor(-0.)", "tensor(-0.2500)", "tensor(inf)"]
    assert len(fallbacks) == 5
    del fallbacks[:]
    vals = torch.tensor([0.5, 0.123456789, 3e-5], dtype=torch.float32)
    torch.set_printoptions(precision=6)
    try:
        got = V._conf_keys(vals)
        want = [str(v) for v in vals]
    finally:
        torch.set_printoptions(profile="default")
    assert got == want and got[1] == "tensor(0.123457)"
    assert len(fallbacks) == 3
    del fallbacks[:]
    assert V._conf_keys(vals) == ["tensor(0.5000)", "tensor(0.1235)", "tensor(3.0000e-05)"] and fallbacks == []


def _validation(**kw):
    params = {"train_params": {"batch_size": 4, "IOU_val_thre": 0.5},
              "io_params": {"input_shape": (256, 320, 1), "num_cls": 3, "class_names": ["carrier", "defender", "destroyer"],
                            "conf_thre": 0.5, "nms_thre": 0.2}}
    frames = [(np.zeros((2, 2, 1), np.float32), np.zeros((64, 6), np.float32))] * 4
    return V.Validation(params, logging.getLogger("t"), frames, "cpu", None, **kw)


def test_match_keyword():
    assert _validation().match == "host" and _validation(match="device").match == "device"
    for bad in ("bogus", None, "Device"):
        with pytest.raises(ValueError):
            _validation(match=bad)


def test_target_num_counts_like_the_loop(golden):
    """`_count_targets` (the vectorised count of device mode) against `_match_image`'s loop: the golden targets, and classes the loop
    wraps around (-1), truncates (1.5) or refuses (num_cls: IndexError in both)."""
    g = golden("golden_map_256")
    val, ref = _validation(match="device"), _validation()
    rec = val._recover_targets(torch.from_numpy(g["targets"]).float())
    odd = rec[:2].clone()
    assert bool((odd[:, :2, 5] > 1).all())
    odd[0, 0, 4], odd[0, 1, 4], odd[1, 0, 4] = -1.0, 1.5, 2.0
    for batch in (rec, odd):
        val.clear(), ref.clear()
        val._count_targets(batch)
        for t in batch:
            ref._match_image(None, t)
        assert val.target_num.tolist() == ref.target_num.tolist() and val.target_num.sum() > 0
    odd[1, 1, 4] = 3.0
    with pytest.raises(IndexError):
        val._count_targets(odd)
    with pytest.raises(IndexError):
        for t in odd:
            ref._match_image(None, t)


def test_val_match_refuses_bad_arguments_before_any_launch():
    lib = _lib.lib()
    buf = (ctypes.c_int64 * 8)()                      # host memory: a call that got past the checks would fail, not be refused
    p = ctypes.addressof(buf)
    good = dict(device=0, det=p, counts=p, N=2, K=4, targets=p, T=3, thres=0.5, base=p, next=p + 8, rec=p, cap=16)

    def call(**kw):
        a = dict(good, **kw)
        return lib.yf_val_match(a["device"], a["det"], a["counts"], a["N"], a["K"], a["targets"], a["T"], a["thres"], a["base"], a["next"],
                                a["rec"], a["cap"], None)
    for name in ("det", "counts", "targets", "base", "next", "rec"):
        assert call(**{name: None}) == _lib.YF_E_INVALID, name
        assert b"null pointer" in lib.yf_last_error_string()
    for kw in (dict(N=0), dict(N=-1), dict(K=0), dict(K=-3), dict(T=-1), dict(cap=-1), dict(T=65537), dict(next=p)):
        assert call(**kw) == _lib.YF_E_INVALID, kw
        assert b"yf_val_match" in lib.yf_last_error_string()
