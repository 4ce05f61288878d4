"""tests/arena.py proven on CPU stand-ins for a kernel: each planted fault is flagged, under exactly the fills that can show it, and a
correct stand-in passes.  The stand-in computes out = 2 * x over n floats; it is handed the arena's raw bytes and its tensors' byte offsets,
as a kernel is handed pointers, so it can reach what lies outside its tensors."""
import re

import pytest
import torch

from tests import arena as ar

N = 1000          # floats: 4000 B, no multiple of the alignment


def _f32(a, off, n):
    return a.raw[off:off + 4 * n].view(torch.float32)


def _off(a, v):
    return v.data_ptr() - a.raw.data_ptr()


def _case(kernel):
    """The stand-in under each fill -> ({fill: complaints of that run alone}, the outputs whose bits differ between the fills)."""
    x = torch.linspace(-3.0, 5.0, N)
    per_fill, results = {}, {}
    for fill in ar.FILLS:
        a = ar.Arena("cpu", fill, ar.room([4 * N, 4 * N]))
        xv, out = a.put(x, "x"), a.empty((N,), torch.float32, "out")
        kernel(a, _off(a, xv), _off(a, out))
        results[fill] = {"out": out.clone(), "x": xv.clone()}
        per_fill[fill] = ar.complaints(a, results[fill], {"out": 2 * x, "x": x})
    return per_fill, ar.differing(results)


def correct(a, x, out):
    _f32(a, out, N).copy_(2 * _f32(a, x, N))


def one_past_the_end(a, x, out):
    correct(a, x, out)
    _f32(a, out, N + 1)[N] = 1.23            # bytes a4 70 9d 3f: none of them 0x00 or 0xff


def zeros_before_the_start(a, x, out):
    correct(a, x, out)
    _f32(a, out - 16, 4).zero_()


def zero_times_guard(a, x, out):
    correct(a, x, out)
    o = _f32(a, out, N)
    o[N - 1] = o[N - 1] + 0.0 * _f32(a, x, N + 1)[N]       # the element behind x, masked by a product


def last_left_unwritten(a, x, out):
    _f32(a, out, N - 1).copy_(2 * _f32(a, x, N - 1))


def flagged(per_fill):
    return {f for f, m in per_fill.items() if m}


def test_layout_guards_and_alignment():
    a = ar.Arena("cpu", "ramp", ar.room([100, 4096], ar.WS_GUARD))
    u = a.take(100, "u")
    w = a.take(4096, "ws", guard=ar.WS_GUARD)
    v = a.take(7, "v")
    base = a.raw.data_ptr()
    assert base % ar.ALIGN == 0 and all(t.data_ptr() % ar.ALIGN == 0 for t in (u, w, v))
    assert u.data_ptr() - base >= ar.GUARD
    assert w.data_ptr() - (u.data_ptr() + 100) >= ar.WS_GUARD and v.data_ptr() - (w.data_ptr() + 4096) >= ar.WS_GUARD
    assert base + a.raw.numel() - (v.data_ptr() + 7) >= ar.GUARD
    assert int(u[0]) == (131 * (u.data_ptr() - base) + 7) & 255 and a.untouched(w) == 4096        # payloads hold the fill too
    a.check()
    spans = a.guards()
    assert spans[0][2] == 0 and spans[-1][3] == a.raw.numel() and all(p[3] <= q[2] for p, q in zip(spans, spans[1:]))
    with pytest.raises(AssertionError, match="exhausted"):
        a.take(a.raw.numel())
    assert torch.isnan(ar.Arena("cpu", "ones", ar.room([8])).empty((2,), torch.float32)).all()
    assert torch.isnan(ar.Arena("cpu", "ones", ar.room([8])).empty((4,), torch.float16)).all()
    assert (ar.Arena("cpu", "ones", ar.room([8])).empty((2,), torch.int32) == -1).all()


def test_a_correct_stand_in_passes():
    per_fill, diff = _case(correct)
    assert flagged(per_fill) == set() and diff == [], per_fill
    x = torch.linspace(-3.0, 5.0, N)

    def run(a):
        xv, out = a.put(x, "x"), a.empty((N,), torch.float32, "out")
        correct(a, _off(a, xv), _off(a, out))
        return {"out": out}
    assert torch.equal(ar.run_fills("cpu", ar.room([4 * N, 4 * N]), run, {"out": 2 * x})["out"], 2 * x)


def test_a_write_one_element_past_the_end_is_flagged_under_every_fill():
    per_fill, _ = _case(one_past_the_end)
    assert flagged(per_fill) == set(ar.FILLS)
    for f in ar.FILLS:
        # the byte written (a4 70 9d 3f) may coincide with the ramp's own byte at the first offsets: under the ramp only "within the element" holds
        assert len(per_fill[f]) == 1 and "after 'out'" in per_fill[f][0], per_fill[f]
        assert "first at 0 B past its end" in per_fill[f][0] or (f == "ramp" and re.search(r"first at [0-3] B past its end", per_fill[f][0])), per_fill[f]


def test_zeros_written_before_the_start_show_under_ones_and_ramp_only():
    per_fill, diff = _case(zeros_before_the_start)
    assert flagged(per_fill) == {"ones", "ramp"} and diff == []
    assert "before 'out'" in per_fill["ones"][0] and "first at 16 B before its start" in per_fill["ones"][0], per_fill["ones"]


def test_zero_times_a_guard_element_shows_under_ones_only():
    # the ramp's element behind x must be finite for the product to vanish there: the layout is deterministic, so this holds or fails for good
    a = ar.Arena("cpu", "ramp", ar.room([4 * N, 4 * N]))
    xv = a.put(torch.zeros(N), "x")
    assert torch.isfinite(_f32(a, _off(a, xv), N + 1)[N])
    per_fill, diff = _case(zero_times_guard)
    assert flagged(per_fill) == {"ones"} and diff == ["out"]
    assert any("non-finite" in m and "flat index %d" % (N - 1) in m for m in per_fill["ones"]), per_fill["ones"]
    assert not any("guard" in m for m in per_fill["ones"])          # nothing was written out of bounds: only the value tells


def test_a_last_element_left_unwritten_is_flagged():
    per_fill, diff = _case(last_left_unwritten)
    assert flagged(per_fill) == set(ar.FILLS) and diff == ["out"]         # against the expected bits: every fill; without them: across fills
    assert any("non-finite" in m for m in per_fill["ones"])
    for f in ("ones", "ramp"):
        a = ar.Arena("cpu", f, ar.room([4 * N]))
        out = a.empty((N,), torch.float32, "out")
        out[:N - 1] = 1.5
        assert a.untouched(out) == 1, f


def test_run_fills_asserts_each_planted_fault():
    x = torch.linspace(-3.0, 5.0, N)
    for kernel in (one_past_the_end, zeros_before_the_start, zero_times_guard, last_left_unwritten):
        def run(a):
            xv, out = a.put(x, "x"), a.empty((N,), torch.float32, "out")
            kernel(a, _off(a, xv), _off(a, out))
            return {"out": out}
        with pytest.raises(AssertionError):
            ar.run_fills("cpu", ar.room([4 * N, 4 * N]), run)         # no expected bits given: containment and the fills alone
