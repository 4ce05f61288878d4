"""TEST INFRASTRUCTURE of test_cpu_optim.py / test_gpu_optim.py: the configurations, tensor layouts and data of the optimizer tests, and
torch.optim.SGD's arithmetic restated in numpy (what csrc/yf_train_opt_kernels.h: tsgd_group_kernel must compute)."""
import numpy as np

SIZES = (1, 3, 255, 256, 257, 1000)          # one element, odd, one short of / exactly / one past a workgroup of 256, several workgroups
CONFIGS = [(0.937, True, 5e-4), (0.937, False, 0.0), (0.0, False, 5e-4), (0.0, False, 0.0), (0.8, True, 0.0)]      # (momentum, nesterov, wd)
STEPS = 5
LATE = 2                                     # index into SIZES of the tensor whose first gradient arrives at step 2
LR_EDIT = 0.37                               # every group's lr is multiplied by this before step 3


def layout(name, wd):
    """-> [(indices into SIZES, lr, weight_decay)] per param group.  "three": different lr and wd per group, the 257-element tensor
    alone in the middle one (the last partial workgroup of its tensor and the boundary of the group lookup on both sides)."""
    if name == "one":
        return [((0, 1, 2, 3, 4, 5), 0.01, wd)]
    return [((0, 1, 2), 0.01, wd), ((4,), 0.003, 1e-3), ((3, 5), 0.02, 0.0)]


def parameters(seed):
    rng = np.random.default_rng(seed)
    out = [rng.normal(size=n).astype(np.float32) for n in SIZES]
    for a in out:
        a[0] = -0.0
    return out


def gradients(seed, it):
    """gradients spanning 1e-6 .. 10, element 0 of every tensor -0.0; None for the late tensor in the first step"""
    rng = np.random.default_rng(1000 * seed + it + 1)
    out = [(rng.normal(size=n) * 10.0 ** rng.uniform(-6, 1, n)).astype(np.float32) for n in SIZES]
    for a in out:
        a[0] = -0.0
    if it == 0:
        out[LATE] = None
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def fma32(a, b, c):
    """float32 fused multiply-add, correctly rounded: the product of two float32 is exact in float64; the sum is rounded to odd there
    (TwoSum tells whether it was inexact), after which the rounding to float32 is the only one that counts (53 >= 24 + 2 bits)."""
    a, b, c = np.broadcast_arrays(*[np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c)])
    x = a * b
    s = x + c
    bb = s - x
    err = (x - (s - bb)) + (c - bb)                                  # x + c == s + err exactly
    even = (np.ascontiguousarray(s).view(np.int64) & 1) == 0
    s = np.where((err != 0) & even, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def sgd_model(p, g, buf, lr, mom, nesterov, wd):
    """One torch.optim.SGD step of one float32 tensor -> (p, momentum buffer or None).  Every scalar is a Python double rounded once to
    float32.  `buf` None = the tensor's first step.  The wd == 0 and first-step branches are not optimisations: fma(0, p, -0.0) and
    0 * mom + (-0.0) give +0.0 where torch keeps -0.0."""
    f = np.float32
    d = fma32(f(wd), p, g) if wd != 0 else g
    if mom != 0:
        buf = d.copy() if buf is None else f(mom) * buf + d          # two float32 operations: a rounded product, then the sum
        d = fma32(f(mom), buf, d) if nesterov else buf
    return fma32(f(-lr), d, p), (buf if mom != 0 else None)
