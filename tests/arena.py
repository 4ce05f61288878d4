"""A guarded, poisoned arena: the memory a kernel under test is handed, so that a result which depends on bytes outside its tensors, or a
write that lands outside them, shows (tests/test_cpu_arena.py proves the helper itself; test_gpu_poison_*.py use it on the device).

`Arena(device, fill, capacity)` owns ONE uint8 allocation, pre-filled as a whole -- payloads and guards alike -- by `fill`:
    zero   0x00
    ones   0xFF: NaN as fp32 and as fp16, -1 as int32
    ramp   byte (131 * i + 7) & 255 at offset i of the arena
`take(nbytes)` carves a view out of it with at least `guard` bytes of fill on either side (GUARD = 64 KiB; WS_GUARD = 1 MiB for a workspace);
everything that is not a payload is guard.  `check()` asserts that every guard byte still holds its fill and names the buffer and the first
offset that does not.  A constant written out of bounds is invisible under the fill it equals, and `0 * garbage` is visible under `ones`
alone: a case therefore runs under ALL of FILLS and asserts containment, finiteness and bitwise equality of its results under each.
Bitwise equality carries most of the weight on the device: a ReLU (fmaxf, or the integer max of the bits on a negative NaN such as 0xFF..)
turns a NaN into 0, so a poisoned operand usually shows as a finite WRONG value, not as a NaN in the result.

Offsets are deterministic: offset 0 of the arena is a 256-byte-aligned address whatever the allocator returned, so a payload sees the same
ramp bytes in every run.  Plain torch: works for CPU and GPU tensors."""
import torch

FILLS = ("zero", "ones", "ramp")
GUARD = 64 << 10
WS_GUARD = 1 << 20
ALIGN = 256


def _up(n, a):
    return (n + a - 1) // a * a


def room(sizes, guard=GUARD, align=ALIGN):
    """Capacity that holds payloads of `sizes` bytes, each with `guard` bytes on either side."""
    return guard + sum(_up(int(n), align) + guard + align for n in sizes)


def same_bits(a, b):
    """Bitwise equality of two tensors of one shape and dtype (NaN == NaN of the same payload)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


class Arena:
    def __init__(self, device, fill, capacity):
        assert fill in FILLS, fill
        self.fill, self.device = fill, torch.device(device)
        self._alloc = torch.empty(int(capacity) + ALIGN, dtype=torch.uint8, device=self.device)
        skew = (-self._alloc.data_ptr()) % ALIGN
        self.raw = self._alloc[skew:skew + int(capacity)]            # offset 0 is ALIGN-aligned
        self.raw.copy_(self.pattern(0, int(capacity)))
        self.bufs = []                                               # (name, start, end) of the payloads, ascending
        self._end, self._tail = 0, 0                                 # end of the last payload, guard owed behind it

    def pattern(self, lo, hi):
        """The fill of arena offsets [lo, hi)."""
        if self.fill == "ramp":                      # period 256: one period, repeated (no int64 index of a workspace's size)
            period = ((torch.arange(256, dtype=torch.int64, device=self.device) * 131 + 7) & 255).to(torch.uint8)
            return period.repeat((hi - lo + 255) // 256 + 1)[lo % 256:lo % 256 + hi - lo]
        return torch.full((hi - lo,), 0 if self.fill == "zero" else 255, dtype=torch.uint8, device=self.device)

    def take(self, nbytes, name=None, guard=GUARD, align=ALIGN):
        """A uint8 view of `nbytes` bytes at an `align`-aligned address, still holding the fill, at least `guard` bytes away from every other
        payload and from both ends of the allocation."""
        nbytes = int(nbytes)
        assert nbytes > 0 and align > 0
        base = self.raw.data_ptr()
        start = max(self._end + guard, self._end + self._tail)
        start = _up(base + start, align) - base
        end = start + nbytes
        assert end + guard <= self.raw.numel(), "arena of %d B exhausted by %r (%d B + %d B guard at %d)" % (self.raw.numel(), name, nbytes, guard, start)
        self.bufs.append((name or "buf%d" % len(self.bufs), start, end))
        self._end, self._tail = end, guard
        return self.raw[start:end]

    def empty(self, shape, dtype, name=None, guard=GUARD):
        """A tensor of `shape` and `dtype` in the arena, holding the fill."""
        shape = tuple(int(s) for s in shape)
        n = 1
        for s in shape:
            n *= s
        return self.take(n * torch.empty((), dtype=dtype).element_size(), name, guard).view(dtype).view(shape)

    def put(self, t, name=None, guard=GUARD):
        """A copy of tensor `t` in the arena."""
        v = self.empty(t.shape, t.dtype, name, guard)
        v.copy_(t)
        return v

    def guards(self):
        """[(name of the nearest payload, side, lo, hi)] of every guard span, in order; the span between two payloads is split at its middle."""
        out, prev = [], None
        for name, start, end in self.bufs:
            if prev is None:
                out.append((name, "before", 0, start))
            else:
                mid = (prev[2] + start) // 2
                out.append((prev[0], "after", prev[2], mid))
                out.append((name, "before", mid, start))
            prev = (name, start, end)
        if prev is not None:
            out.append((prev[0], "after", prev[2], self.raw.numel()))
        else:
            out.append(("arena", "in", 0, self.raw.numel()))
        return out

    def broken(self):
        """None, or a description of the first guard byte that no longer holds its fill."""
        for name, side, lo, hi in self.guards():
            if hi <= lo:
                continue
            bad = self.raw[lo:hi] != self.pattern(lo, hi)
            if bool(bad.any()):
                first = int(bad.nonzero()[0, 0])
                start, end = next((s, e) for n, s, e in self.bufs if n == name) if self.bufs else (0, 0)
                where = "%d B before its start" % (start - (lo + first)) if side == "before" else "%d B past its end" % (lo + first - end)
                return "fill %s: guard %s %r overwritten, first at %s (arena offset %d, %d bytes differ in this span, byte 0x%02x)" % (
                    self.fill, side, name, where, lo + first, int(bad.sum()), int(self.raw[lo + first]))
        return None

    def check(self):
        msg = self.broken()
        assert msg is None, msg

    def untouched(self, view):
        """How many elements of a payload view still hold, in every byte, the fill they were handed with: under `ones` and `ramp` the elements
        nobody wrote (under `zero` an honest 0 counts too)."""
        lo = view.data_ptr() - self.raw.data_ptr()
        n = view.numel() * view.element_size()
        assert 0 <= lo and lo + n <= self.raw.numel() and view.is_contiguous()
        return int((self.raw[lo:lo + n] == self.pattern(lo, lo + n)).view(-1, view.element_size()).all(dim=1).sum())


def complaints(arena, outs, want=None):
    """What one run under one fill shows: a broken guard, a float result that is not finite, a result whose bits differ from `want`'s
    ({name: tensor}, optional, for the names it holds).  outs: {name: tensor}.  Returns a list of strings, empty when the run is clean."""
    msgs = []
    g = arena.broken()
    if g:
        msgs.append(g)
    for name, t in outs.items():
        if t.is_floating_point() and not bool(torch.isfinite(t).all()):
            bad = (~torch.isfinite(t)).flatten().nonzero()
            msgs.append("fill %s: %s has %d non-finite elements, first at flat index %d" % (arena.fill, name, bad.numel(), int(bad[0, 0])))
        if want is not None and name in want and not same_bits(t, want[name].to(t.device)):
            d = (t.contiguous().view(torch.uint8) != want[name].to(t.device).contiguous().view(torch.uint8)).flatten().nonzero() \
                if t.shape == want[name].shape and t.dtype == want[name].dtype else None
            msgs.append("fill %s: %s differs from the expected bits%s" % (arena.fill, name, "" if d is None else ", first at byte %d" % int(d[0, 0])))
    return msgs


def differing(results):
    """results: {fill: {name: tensor}} of one case -> the names whose bits are not the same under every fill."""
    fills = list(results)
    return [n for n in results[fills[0]] if not all(same_bits(results[fills[0]][n], results[f][n]) for f in fills[1:])]


def run_fills(device, capacity, run, want=None):
    """`run(arena) -> {name: tensor}` under each of FILLS, results cloned out of the arena after a device synchronisation.  Asserts
    containment under each fill (guards, finite results, `want`'s bits where given) and bitwise equality across the fills; returns the
    results of the `zero` run."""
    results, msgs = {}, []
    for fill in FILLS:
        a = Arena(device, fill, capacity)
        outs = run(a)
        if a.device.type == "cuda":
            torch.cuda.synchronize(a.device)
        results[fill] = {n: t.clone() for n, t in outs.items()}
        msgs += complaints(a, results[fill], want)
        del a, outs
    msgs += ["%s: bits differ between the fills" % n for n in differing(results)]
    assert not msgs, "\n".join(msgs)
    return results["zero"]
