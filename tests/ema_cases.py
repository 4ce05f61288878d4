"""TEST INFRASTRUCTURE of test_cpu_ema.py / test_gpu_ema.py: the tensors, decays and toy module of the ModelEMA tests, and yolov5's update
restated in numpy float32 (what csrc/yf_train_opt_kernels.h: tema_update must compute): e = round(round(e d) + round((1 - d) p))."""
import math

import numpy as np

from optim_cases import bits, fma32

SIZES = (1, 255, 256, 257, 513, 1000)        # the edges of a 256-thread workgroup on both sides, two and four workgroups
DECAY, TAU = 0.9999, 2000                    # ModelEMA's defaults
UPDATES = (1, 2, 2000, 10 ** 6)              # d ~ 5e-4, 1e-3, 0.632, -> 0.9999


def ramp(updates, decay=DECAY, tau=TAU):
    """ModelEMA.decay in closed form, in double"""
    return decay * (1.0 - math.exp(-updates / tau))


def d_values():
    """the default ramp at UPDATES, then the edges d = 0 (the average becomes the model) and d = 1 (it stays)"""
    return [ramp(u) for u in UPDATES] + [0.0, 1.0]


def ema_model(e, p, d):
    """One update of one float32 tensor: three float32 operations, each rounded; d and 1 - d are Python doubles rounded once."""
    f = np.float32
    e, p = np.asarray(e, f), np.asarray(p, f)
    with np.errstate(all="ignore"):
        return (e * f(d)) + (f(1.0 - d) * p)


def fused_models(e, p, d):
    """What a compiler that contracts the sum into a fused multiply-add would compute, either way round"""
    f = np.float32
    e, p = np.asarray(e, f), np.asarray(p, f)
    with np.errstate(all="ignore"):
        return fma32(e, f(d), f(1.0 - d) * p), fma32(f(1.0 - d), p, e * f(d))


FMA_CASE = 2                                 # index into cases() of the block chosen against contraction


def cases():
    """-> [(name, e, p)]: one (EMA, model) pair of float32 tensors per entry of SIZES, in the order of one multi-tensor call.
    normals; the block where a fused multiply-add rounds differently; signed zeros; subnormals; infinities; magnitudes 1e-30 .. 1e30."""
    rng = np.random.default_rng(20240)
    f = np.float32

    def normal(n):
        return rng.normal(size=n).astype(f)
    out = [("normal-1", normal(1), normal(1)), ("normal-255", normal(255), normal(255))]
    # 64 pairs for each of the ramp's four d at which BOTH fused forms differ from multiply-then-add, picked from a seeded pool whose
    # e spans eight decades (at d ~ 5e-4 the two products are of one magnitude, and the rounding of either matters, only when e >> p)
    e, p = (rng.normal(size=1 << 16) * 10.0 ** rng.uniform(-4, 4, 1 << 16)).astype(f), normal(1 << 16)
    pick = []
    for u in UPDATES:
        a, b = fused_models(e, p, ramp(u))
        want = ema_model(e, p, ramp(u))
        pick.append(np.nonzero((bits(a) != bits(want)) & (bits(b) != bits(want)))[0][:64])
        assert len(pick[-1]) == 64, u
    pick = np.concatenate(pick)
    out.append(("fma-256", e[pick].copy(), p[pick].copy()))
    z = np.array([0.0, -0.0, 0.0, -0.0, 1.5, -1.5, 0.0, -0.0], f)
    zp = np.array([0.0, 0.0, -0.0, -0.0, 0.0, -0.0, 2.5, -2.5], f)
    e, p = normal(257), normal(257)
    e[:8], p[:8] = z, zp
    e[-8:], p[-8:] = z, zp                                          # (the last one: the tensor's second, one-thread workgroup)
    out.append(("zeros-257", e, p))
    tiny = f(2.0 ** -149)
    e = (rng.integers(-(2 ** 23) + 1, 2 ** 23, 513).astype(f) * tiny).astype(f)          # every exponent-0 pattern: subnormals and zeros
    p = (rng.integers(-(2 ** 23) + 1, 2 ** 23, 513).astype(f) * tiny).astype(f)
    p[::7] = normal(len(p[::7])) * f(1e-38)                          # around the smallest normal: results that cross the boundary
    assert np.all(np.abs(e) < np.finfo(f).tiny)
    out.append(("subnormal-513", e, p))
    e = (rng.normal(size=1000) * 10.0 ** rng.uniform(-30, 30, 1000)).astype(f)
    p = (rng.normal(size=1000) * 10.0 ** rng.uniform(-30, 30, 1000)).astype(f)
    inf = f(np.inf)
    e[:6] = [inf, -inf, inf, 1.0, -1.0, inf]                         # inf - inf and 0 * inf give NaN: left out of the bit comparisons
    p[:6] = [1.0, -1.0, -inf, inf, -inf, inf]
    e[-3:], p[-3:] = [inf, 3e38, -3e38], [2.0, 3e38, -3e38]          # finite operands whose sum may overflow
    out.append(("magnitudes-inf-1000", e, p))
    assert tuple(len(c[1]) for c in out) == SIZES
    return out


def same_bits_or_nan(got, want):
    """bit equality wherever `want` is a number; NaN where it is not (which NaN is nobody's contract)"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan]))


def toy_module(arrays, torch):
    """A module whose floating state-dict entries are `arrays` as parameters p0, p1, ..., a float buffer `stat` (a running statistic:
    no gradient, ever) and an integer buffer `count` (not averaged).  Its forward returns [the sum of the parameters' squares]."""
    class Toy(torch.nn.Module):
        def __init__(self):
            super().__init__()
            for i, a in enumerate(arrays):
                self.register_parameter("p%d" % i, torch.nn.Parameter(torch.from_numpy(np.array(a, np.float32))))
            self.register_buffer("stat", torch.linspace(-2.0, 3.0, 300))
            self.register_buffer("count", torch.tensor(7))

        def forward(self, x=None):                                   # one "head": something for a backward to start from
            return [sum((p * p).sum() for p in self.parameters())]
    return Toy()
