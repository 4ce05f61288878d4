"""A seeded progressive JPEG writer in numpy (test infrastructure): the scan scripts PIL's encoder never writes, for
tests/test_cpu_jpeg_prog.py and tests/test_gpu_jpeg_prog.py.  It takes planes, quantisation, optimal tables, canonical codes and the bit
packing from tests/jpeg_write.py, so `baseline(...)` (that file's encoder with the same settings) holds the same coefficients.

A script is a list of scans (components, Ss, Se, Ah, Al) in file order.  Any complete script can be written: DC and AC in any band split,
Al from 0 to 13 with any number of refinement passes, interleaved and non-interleaved DC scans (also two of three components), chroma
before luma.  Encoding follows ITU-T T.81 Annex G: DC first (arithmetic shift by Al, differences), DC refinement (one bit), AC first
(magnitude >> Al, run / size, ZRL, EOBn runs up to 32767 blocks), AC refinement (correction bits buffered behind the next symbol, new +-1
coefficients, ZRL only in front of a later new coefficient, EOB runs that carry correction bits).  Every scan gets tables optimised from
its own symbol counts (Annex K.2), written in front of it (so tables are redefined between scans), optionally merged into one DHT or
first defined with other contents; DRI may change between scans; fill bytes may stand before RSTn and other markers; restart intervals
count the scan's own MCUs (a non-interleaved scan walks the component's real blocks only).  Corruption hooks make the device decoder's
status flags on purpose."""
import numpy as np

import jpeg_write as jw

ZRL = 0xF0


def pillow_script(nc):
    """libjpeg's jpeg_simple_progression."""
    if nc == 1:
        return [((0,), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1), ((0,), 0, 0, 1, 0), ((0,), 1, 63, 1, 0)]
    return [((0, 1, 2), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((2,), 1, 63, 0, 1), ((1,), 1, 63, 0, 1), ((0,), 6, 63, 0, 2),
            ((0,), 1, 63, 2, 1), ((0, 1, 2), 0, 0, 1, 0), ((2,), 1, 63, 1, 0), ((1,), 1, 63, 1, 0), ((0,), 1, 63, 1, 0)]


def scripts(nc):
    """{name: script}: the test matrix of scan scripts for a frame of `nc` components."""
    comps = list(range(nc))
    allc = tuple(comps)
    out = {"pillow": pillow_script(nc)}
    # spectral selection only, bands split three ways, DC interleaved
    out["spectral"] = [(allc, 0, 0, 0, 0)] + [((c,), a, b, 0, 0) for c in comps for a, b in ((1, 1), (2, 9), (10, 63))]
    # successive approximation only: DC not interleaved, deep AC refinement chains; chroma first
    order = comps[::-1]
    out["deep"] = ([((c,), 0, 0, 0, 2) for c in order] + [((c,), 1, 63, 0, 3) for c in order]
                   + [((c,), 1, 63, ah, ah - 1) for ah in (3, 2, 1) for c in order] + [((c,), 0, 0, ah, ah - 1) for ah in (2, 1) for c in order])
    # Al = 13 down to 0 in 13 refinement passes, DC and one AC band; the rest of the spectrum in one scan
    out["al13"] = ([(allc, 0, 0, 0, 13)] + [(allc, 0, 0, ah, ah - 1) for ah in range(13, 0, -1)]
                   + [((c,), 1, 3, 0, 13) for c in comps] + [((c,), 1, 3, ah, ah - 1) for ah in range(13, 0, -1) for c in comps]
                   + [((c,), 4, 63, 0, 0) for c in comps])
    # one long chain: every AC scan refines the one before it (one scan per level behind the two first scans)
    out["chain"] = [((0,), 0, 0, 0, 0), ((0,), 1, 63, 0, 4)] + [((0,), 1, 63, ah, ah - 1) for ah in (4, 3, 2, 1)]
    if nc == 3:
        out["chain"] += [((1, 2), 0, 0, 0, 0), ((1,), 1, 63, 0, 0), ((2,), 1, 63, 0, 0)]
        # DC of two components interleaved, the third alone; mixed
        out["pairs"] = [((0,), 0, 0, 0, 1), ((1, 2), 0, 0, 0, 0), ((0,), 0, 0, 1, 0), ((2,), 1, 63, 0, 1), ((1,), 1, 20, 0, 0),
                        ((0,), 1, 63, 0, 1), ((1,), 21, 63, 0, 0), ((2,), 1, 63, 1, 0), ((0,), 1, 63, 1, 0)]
    return out


def coefficients(a, layout="420", quality=75, rgb=False):
    """([by, bx, 64] int coefficients in zig-zag order per component (MCU-padded), quantisation tables in zig-zag order per component)."""
    std = jw.standard_tables()
    nc = 1 if layout == "gray" else 3
    qt = [jw.scaled_qtable(std["q"][0 if c == 0 else 1], quality) for c in range(nc)]
    ps = jw.planes(a, layout, rgb)
    return [jw.quantise(p, qt[c]) for c, p in enumerate(ps)], qt


def baseline(a, layout="420", quality=75, **kw):
    """The baseline file of the same coefficients (tests/jpeg_write.py)."""
    return jw.encode(a, layout, quality, **kw)


def _nbits(v):
    return int(v).bit_length()


class _Scan:
    """The token stream of one scan: ('s', symbol, table slot) Huffman symbols, ('b', value, nbits) raw bits, ('r',) restart boundaries."""

    def __init__(self):
        self.tok = []
        self.eobrun = 0
        self.be = []                       # correction bits waiting behind the pending EOB run
        self.slot = 0

    def sym(self, s):
        self.tok.append(("s", s, self.slot))

    def bits(self, v, n):
        if n:
            self.tok.append(("b", int(v), n))

    def flush_eobrun(self):
        if self.eobrun > 0:
            n = _nbits(self.eobrun) - 1
            self.sym(n << 4)
            self.bits(self.eobrun & ((1 << n) - 1), n)
            self.eobrun = 0
            for b in self.be:
                self.bits(b, 1)
            self.be = []


def _ac_first(sc, blk, ss, se, al, max_run):
    r = 0
    nz = [k for k in range(ss, se + 1) if blk[k]]
    prev = ss - 1
    for k in nz:
        t = abs(blk[k]) >> al
        if t == 0:
            continue
        r = k - prev - 1
        prev = k
        sc.flush_eobrun()
        while r > 15:
            sc.sym(ZRL)
            r -= 16
        n = _nbits(t)
        sc.sym((r << 4) | n)
        sc.bits(t if blk[k] > 0 else (1 << n) - 1 - t, n)
    if prev < se:
        sc.eobrun += 1
        if sc.eobrun == max_run:
            sc.flush_eobrun()


def _ac_refine(sc, blk, ss, se, al, max_run):
    absv = [abs(v) >> al for v in blk[ss:se + 1]]
    eob = max([i for i, t in enumerate(absv) if t == 1] or [-1])
    r, br = 0, []
    for i, t in enumerate(absv):
        if t == 0:
            r += 1
            continue
        while r > 15 and i <= eob:
            sc.flush_eobrun()
            sc.sym(ZRL)
            r -= 16
            for b in br:
                sc.bits(b, 1)
            br = []
        if t > 1:
            br.append(t & 1)
            continue
        sc.flush_eobrun()
        sc.sym((r << 4) | 1)
        sc.bits(0 if blk[ss + i] < 0 else 1, 1)
        for b in br:
            sc.bits(b, 1)
        br, r = [], 0
    if r > 0 or br:
        sc.eobrun += 1
        sc.be += br
        if sc.eobrun == max_run or len(sc.be) > 937:
            sc.flush_eobrun()


def encode(a, layout="420", quality=75, script=None, *, rgb=False, ri=0, fill=0, marker_fill=0, dht="split", redefine=False, max_run=0x7FFF,
           late_dqt=False, truncate_scan=None, ones_scan=None, drop_rst=None, extra_rst=None, run_past_se=None, sof=0xC2, precision=8):
    """Progressive JPEG bytes of `a` (uint8 [h, w, 3], or [h, w] / channel 0 for gray) with scan script `script` (default: Pillow's).

    ri: restart interval in the scan's own MCUs, one int for every scan or a list per scan (DRI is rewritten when it changes).  fill:
    0xFF fill bytes before each RSTn; marker_fill: before the DHT / DRI / SOS / EOI markers that follow entropy-coded data.  dht: 'split'
    (one segment per table) or 'merged' (a scan's tables in one).  redefine: each table is first defined with other contents.  max_run:
    longest EOB run (T.81: 32767).  late_dqt: the chroma quantisation table arrives only before the first scan that names a chroma
    component, and after that scan every table is redefined with other contents (which a decoder must not pick up).  sof / precision: the
    frame header's marker and sample precision (refusal tests).
    Corruption: truncate_scan = i: scan i's bytes cut in half; ones_scan = i: 128 bytes in its middle replaced by stuffed 0xFF;
    drop_rst / extra_rst = (i, j): the RSTn after interval j of scan i left out / written twice; run_past_se = i: the first block of AC
    first scan i is coded as ZRLs and a run that ends one past Se."""
    a = np.asarray(a)
    h, w = a.shape[:2]
    nc = 1 if layout == "gray" else 3
    hs, vs = jw.SAMPLING[layout]
    samp = [(hs, vs)] + [(1, 1)] * (nc - 1)
    co, qt = coefficients(a, layout, quality, rgb)
    script = list(script if script is not None else pillow_script(nc))
    ris = list(ri) if isinstance(ri, (list, tuple)) else [ri] * len(script)
    mcux, mcuy = jw.mcu_counts(w, h, layout)
    dw = [-(-w * samp[c][0] // hs) for c in range(nc)]
    dh = [-(-h * samp[c][1] // vs) for c in range(nc)]

    out = bytearray(b"\xff\xd8")

    def seg(marker, payload, after_data=False):
        out.extend(b"\xff" * (marker_fill if after_data else 0) + bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload))
    if not rgb:
        seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")

    def dqt(t, vals):
        seg(0xDB, bytes([t]) + bytes(vals))
    dqt(0, qt[0])
    if nc == 3 and not late_dqt:
        dqt(1, qt[1])
    sofp = bytes([precision]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([nc])
    ids = [82, 71, 66] if rgb else [1, 2, 3]
    for c in range(nc):
        sofp += bytes([ids[c], (samp[c][0] << 4) | samp[c][1], 0 if c == 0 else 1])
    seg(sof, sofp)

    cur_ri, chroma_q, named, requantised = 0, not late_dqt, set(), False
    for si, (comps, ss, se, ah, al) in enumerate(script):
        comps = tuple(comps)
        sri = ris[si]
        sc = _Scan()
        # the scan's MCUs: (component position in the scan, by, bx) per block
        if len(comps) == 1:
            c = comps[0]
            bw_, bh_ = -(-dw[c] // 8), -(-dh[c] // 8)
            mcus = [[(0, y, x)] for y in range(bh_) for x in range(bw_)]
        else:
            mcus = [[(j, my * samp[c][1] + y, mx * samp[c][0] + x) for j, c in enumerate(comps) for y in range(samp[c][1])
                     for x in range(samp[c][0])] for my in range(mcuy) for mx in range(mcux)]
        pred = [0] * len(comps)
        first_block = True
        for m, blocks in enumerate(mcus):
            if sri and m and m % sri == 0:
                sc.flush_eobrun()
                sc.tok.append(("r",))
                pred = [0] * len(comps)
            for j, by, bx in blocks:
                blk = co[comps[j]][by, bx].tolist() + [0]          # one past the end: a script with Se = 64 (refusal tests)
                sc.slot = 0 if ss else (0 if comps[j] == 0 else 1)
                if ss == 0 and ah == 0:
                    v = blk[0] >> al
                    d = v - pred[j]
                    pred[j] = v
                    n = _nbits(abs(d))
                    sc.sym(n)
                    sc.bits(d if d >= 0 else d + (1 << n) - 1, n)
                elif ss == 0:
                    sc.bits((blk[0] >> al) & 1, 1)
                elif ah == 0:
                    if si == run_past_se and first_block:
                        for _ in range((se - ss) // 16):
                            sc.sym(ZRL)
                        r = (se - ss) % 16 + 1
                        assert r <= 15
                        sc.sym((r << 4) | 1)
                        sc.bits(1, 1)
                    else:
                        _ac_first(sc, blk, ss, se, al, max_run)
                else:
                    _ac_refine(sc, blk, ss, se, al, max_run)
                first_block = False
        sc.flush_eobrun()

        # tables from the scan's own counts; ids: DC 0 luma / 1 chroma, AC likewise
        if late_dqt and nc == 3 and not chroma_q and any(c > 0 for c in comps):
            dqt(1, qt[1])
            chroma_q = True
        tc = 1 if ss else 0
        freq = {}
        for t in sc.tok:
            if t[0] == "s":
                freq.setdefault(t[2] if not ss else 0, {}).setdefault(t[1], 0)
                freq[t[2] if not ss else 0][t[1]] += 1
        th_of = {}
        if ss:
            th_of[0] = 0 if comps[0] == 0 else 1
        else:
            th_of = {0: 0, 1: 1}
        codes, pays = {}, []
        for slot in sorted(freq):
            table = jw.optimal_table(freq[slot])
            codes[slot] = jw.canonical(*table)
            th = th_of[slot]
            if redefine:
                std = jw.standard_tables()
                alt = std["ac" if tc else "dc"][th]
                seg(0xC4, bytes([(tc << 4) | th] + list(alt[0]) + list(alt[1])), si > 0)
            pays.append(bytes([(tc << 4) | th] + list(table[0]) + list(table[1])))
        if dht == "merged" and pays:
            seg(0xC4, b"".join(pays), si > 0)
        else:
            for p in pays:
                seg(0xC4, p, si > 0)
        if sri != cur_ri:
            seg(0xDD, sri.to_bytes(2, "big"), si > 0)
            cur_ri = sri
        sos = bytes([len(comps)])
        for c in comps:
            th = 0 if c == 0 else 1
            sos += bytes([ids[c], (th << 4) | th])
        seg(0xDA, sos + bytes([ss, se, (ah << 4) | al]), si > 0)

        # entropy-coded bytes
        data = bytearray()
        parts, j = [], 0

        def flush_interval(last):
            nonlocal parts, j
            data.extend(jw._segment_bytes("".join(parts)))
            parts = []
            if not last:
                mk = b"\xff" * fill + bytes([0xFF, 0xD0 + j % 8])
                if drop_rst == (si, j):
                    mk = b""
                elif extra_rst == (si, j):
                    mk = mk + bytes([0xFF, 0xD0 + (j + 1) % 8])
                data.extend(mk)
            j += 1
        for t in sc.tok:
            if t[0] == "s":
                code, ln = codes[t[2] if not ss else 0][t[1]]
                parts.append(format(code, "0%db" % ln))
            elif t[0] == "b":
                parts.append(format(t[1], "0%db" % t[2]))
            else:
                flush_interval(False)
        flush_interval(True)
        if si == truncate_scan:
            data = data[:len(data) // 2]
            while data and data[-1] == 0xFF:
                data = data[:-1]
        if si == ones_scan:
            mid = max(0, len(data) // 2 - 64)
            data = data[:mid] + b"\xff\x00" * 64 + data[mid + 128:]
        out.extend(data)
        named |= set(comps)
        if late_dqt and len(named) == nc and not requantised:   # every component's table is latched: other contents under both indices
            requantised = True
            dqt(0, [min(255, v + 7) for v in qt[0]])
            if nc == 3:
                dqt(1, [min(255, v + 9) for v in qt[1]])
    out.extend(b"\xff" * marker_fill + b"\xff\xd9")
    return bytes(out)
