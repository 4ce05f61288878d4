"""A CPU restatement of the speculative synchronisation of jpeg_entropy_kernel (csrc/yf_jpeg_kernels.hip) for files without restart
markers, to count its rounds (test infrastructure; tests/test_gpu_jpeg_bitstreams.py).

As in the kernel: the scan is de-stuffed into a clean stream (stuffed zeros, fill bytes and RSTn out) that reads as zero bits past its
end; it is cut into 64 equal runs of bits; every lane decodes its run from a guessed state (block 0 of an MCU, DC next) up to the first
symbol boundary at or past the next run's start; then, round after round, a lane whose start state (bit position, block in the MCU,
zig-zag index) differs from its left neighbour's end state takes that state and decodes again, until no start state changes.  A bad code
advances one bit (DC: as category 0; AC: as an end of block), an index past 63 is clamped, as in the kernel."""
import numpy as np

LANES = 64


def _segments(d):
    i, out = 2, []
    while True:
        while d[i + 1] == 0xFF:
            i += 1
        m, ln = d[i + 1], (d[i + 2] << 8) | d[i + 3]
        out.append((m, d[i + 4:i + 2 + ln]))
        i += 2 + ln
        if m == 0xDA:
            return out, i


def _lut(bits, vals):
    """16-bit window -> (code length, symbol); length 0: no code."""
    ln = np.zeros(1 << 16, np.int64)
    sym = np.zeros(1 << 16, np.int64)
    code, p = 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            lo = code << (16 - length)
            hi = lo + (1 << (16 - length))
            ln[lo:hi] = length
            sym[lo:hi] = vals[p]
            code += 1
            p += 1
        code <<= 1
    return ln.tolist(), sym.tolist()


def scan_data(d, start):
    """The entropy-coded bytes as yf_jpeg_pack cuts them: up to the first marker other than a stuffed zero, a fill byte or RSTn."""
    i, n = start, len(d)
    while i < n:
        if d[i] == 0xFF and i + 1 < n:
            m = d[i + 1]
            if m == 0x00 or 0xD0 <= m <= 0xD7:
                i += 2
                continue
            if m == 0xFF:
                i += 1
                continue
            break
        i += 1
    return d[start:i]


def clean_stream(data):
    """The kernel's de-stuffing: 0xFF kept only before 0x00, the 0x00 after 0xFF and RSTn dropped."""
    b = np.frombuffer(data, np.uint8).astype(np.int64)
    prev = np.concatenate([[0], b[:-1]])
    nxt = np.concatenate([b[1:], [-1]])
    keep = np.where(b == 0xFF, nxt == 0x00, ~((prev == 0xFF) & ((b == 0x00) | ((b >= 0xD0) & (b <= 0xD7)))))
    return b[keep].astype(np.uint8)


class Frame:
    """The block layout and tables of one baseline file, its clean stream as 16-bit windows at every bit position."""

    def __init__(self, d):
        segs, start = _segments(d)
        tables, sof = {}, None
        for m, s in segs:
            k = 0
            while m == 0xC4 and k < len(s):
                bits = list(s[k + 1:k + 17])
                tables[(s[k] >> 4, s[k] & 15)] = _lut(bits, list(s[k + 17:k + 17 + sum(bits)]))
                k += 17 + sum(bits)
            if m in (0xC0, 0xC1):
                sof = s
            if m == 0xDD and s[0] << 8 | s[1]:
                raise ValueError("restart markers: every lane starts exact, there are no rounds")
        sos = segs[-1][1]
        h, w, nf = (sof[1] << 8) | sof[2], (sof[3] << 8) | sof[4], sof[5]
        samp = {sof[6 + 3 * c]: (sof[7 + 3 * c] >> 4, sof[7 + 3 * c] & 15) for c in range(nf)}
        self.blocks = []                                     # (DC table, AC table) of every block of an MCU
        for s in range(sos[0]):
            cid, td = sos[1 + 2 * s], sos[2 + 2 * s]
            nb = 1 if nf == 1 else samp[cid][0] * samp[cid][1]
            self.blocks += [(tables[(0, td >> 4)], tables[(1, td & 15)])] * nb
        if nf == 1:
            self.nmcu = -(-w // 8) * -(-h // 8)
        else:
            hm, vm = max(v[0] for v in samp.values()), max(v[1] for v in samp.values())
            self.nmcu = -(-w // (8 * hm)) * -(-h // (8 * vm))
        clean = clean_stream(scan_data(d, start))
        self.total_bits = 8 * len(clean)
        bits = np.concatenate([np.unpackbits(clean).astype(np.int64), np.zeros(64, np.int64)])
        win = np.zeros(self.total_bits + 32, np.int64)
        for i in range(16):
            win += bits[i:i + self.total_bits + 32] << (15 - i)
        self.win = win.tolist()

    def window(self, pos):
        return self.win[pos] if pos < len(self.win) else 0

    def decode(self, pos, blk, k, stop):
        """Decodes from state (pos, blk, k) to the first symbol boundary at or past `stop` -> (end state, MCUs completed)."""
        mcus, bpm = 0, len(self.blocks)
        while pos < stop:
            dc, ac = self.blocks[blk]
            wnd = self.window(pos)
            if k == 0:
                ln, s = dc[0][wnd], dc[1][wnd]
                if not ln:
                    ln, s = 1, 0
                pos += ln + s
                k = 1
            else:
                ln, sym = ac[0][wnd], ac[1][wnd]
                if not ln:
                    pos += 1
                    k = 64
                else:
                    pos += ln
                    rr, s = sym >> 4, sym & 15
                    if s:
                        k = min(k + rr, 63) + 1
                        pos += s
                    elif rr == 15:
                        k += 16
                    else:
                        k = 64
            if k >= 64:
                k = 0
                blk += 1
                if blk == bpm:
                    blk = 0
                    mcus += 1
        return (pos, blk, k), mcus


def sync(d, max_rounds=None):
    """The kernel's round loop on one file -> dict(rounds: decode rounds until no start state changed, mcus: per-lane MCUs of the
    final states, mcus63_at63: lane 63's MCU count had the loop stopped after 63 rounds, nmcu, exact: the final starts are the true
    symbol boundaries of a serial decode)."""
    f = Frame(d)
    tb = f.total_bits
    stops = [tb * (lane + 1) // LANES if lane + 1 < LANES else tb for lane in range(LANES)]
    cur = [(tb * lane // LANES, 0, 0) for lane in range(LANES)]
    ends, mcus = [None] * LANES, [0] * LANES
    redo = [True] * LANES
    history = []
    rounds = 0
    for rnd in range(max_rounds or 10 * LANES):
        for lane in range(LANES):
            if redo[lane]:
                ends[lane], mcus[lane] = f.decode(*cur[lane], stops[lane])
        history.append(mcus[LANES - 1])
        rounds = rnd + 1
        changed = [False] + [ends[lane - 1] != cur[lane] for lane in range(1, LANES)]
        cur = [cur[0]] + [ends[lane - 1] for lane in range(1, LANES)]
        redo = changed
        if not any(changed):
            break
    serial, state = [cur[0]], cur[0]
    for lane in range(LANES - 1):
        state, _ = f.decode(*state, stops[lane])
        serial.append(state)
    return dict(rounds=rounds, mcus=mcus, nmcu=f.nmcu, exact=serial == cur,
                mcus63_at63=history[min(len(history), LANES - 1) - 1], mcu0_63=sum(mcus[:LANES - 1]))
