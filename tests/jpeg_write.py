"""A seeded baseline JPEG writer in numpy (test infrastructure): the streams PIL's encoder never writes, for tests/test_cpu_jpeg_write.py
and tests/test_gpu_jpeg_bitstreams.py.

It covers gray, 4:4:4, 4:2:2, 4:2:0 and 4:4:0 (luma 1 x 2); JFIF / Adobe / bare colour signalling with free component IDs; 8-bit DQT
with SOF0 or 16-bit DQT with SOF1; any table index 0..3 per component; the Annex K Huffman tables or tables optimised from the data
(Annex K.2, 16-bit limit); split, merged or redefined DHT segments; DRI with any interval, fill bytes before RSTn and EOI, extra APPn / COM
segments and trailing bytes.  Corruption hooks make the status flags of the device decoder on purpose.

Encoding: float forward DCT, rounding quantisation clamped so dequantised coefficients stay in the range 8-bit samples produce, DC
categories, AC run / size with ZRL and EOB, byte stuffing, 1-bit padding, RSTn numbered mod 8 and DC predictors reset at each restart.
Chroma is box-downsampled; partial MCUs are padded by edge replication."""
import io

import numpy as np
from PIL import Image

SAMPLING = {"gray": (1, 1), "444": (1, 1), "422": (2, 1), "420": (2, 2), "440": (1, 2)}     # luma (h, v); chroma is 1 x 1
LAYOUTS = list(SAMPLING)

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54,
                   47, 55, 62, 63])                                   # zig-zag index -> natural index

_STD = None


def _segments(d):
    """(marker, payload) of every segment before SOS."""
    out, i = [], 2
    while i < len(d):
        m = d[i + 1]
        ln = (d[i + 2] << 8) | d[i + 3]
        out.append((m, d[i + 4:i + 2 + ln]))
        if m == 0xDA:
            break
        i += 2 + ln
    return out


def standard_tables():
    """{'q': [luma, chroma] base tables in zig-zag order (Annex K.1, quality 50 = scale 100 %), 'dc' / 'ac': [luma, chroma] as
    (bits[1..16], values)}: the Annex K tables, read back from what libjpeg writes for a non-optimised encode."""
    global _STD
    if _STD is None:
        b = io.BytesIO()
        Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(b, "JPEG", quality=50, subsampling=0)
        q, h = {}, {}
        for m, s in _segments(b.getvalue()):
            k = 0
            while m == 0xDB and k < len(s):
                q[s[k] & 15] = list(s[k + 1:k + 65])
                k += 65
            while m == 0xC4 and k < len(s):
                bits = list(s[k + 1:k + 17])
                h[(s[k] >> 4, s[k] & 15)] = (bits, list(s[k + 17:k + 17 + sum(bits)]))
                k += 17 + sum(bits)
        _STD = {"q": [q[0], q[1]], "dc": [h[(0, 0)], h[(0, 1)]], "ac": [h[(1, 0)], h[(1, 1)]]}
    return _STD


def scaled_qtable(base, quality):
    """IJG quality scaling (jpeg_quality_scaling + jpeg_add_quant_table with force_baseline)."""
    quality = min(max(quality, 1), 100)
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return [min(max((v * scale + 50) // 100, 1), 255) for v in base]


def optimal_table(freq):
    """Annex K.2 (libjpeg's jpeg_gen_optimal_table): code lengths from symbol counts {symbol: count}, a reserved all-ones code, lengths
    limited to 16 -> (bits[1..16], values)."""
    f = [0] * 257
    for s, c in freq.items():
        f[s] = c
    f[256] = 1
    codesize, others = [0] * 257, [-1] * 257
    while True:
        c1, v = -1, None
        for i in range(257):
            if f[i] and (v is None or f[i] <= v):
                v, c1 = f[i], i
        c2, v = -1, None
        for i in range(257):
            if f[i] and i != c1 and (v is None or f[i] <= v):
                v, c2 = f[i], i
        if c2 < 0:
            break
        f[c1] += f[c2]
        f[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    bits = [0] * 33
    for i in range(257):
        if codesize[i]:
            bits[codesize[i]] += 1
    for i in range(32, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1                                                    # the reserved code
    vals = [s for size in range(1, 33) for s in range(256) if codesize[s] == size]
    return bits[1:17], vals


def fib_ranked(freq):
    """Counts replaced by Fibonacci numbers in order of rank: K.2 then builds codes deeper than 16 bits and the limiter has to act."""
    a, b, out = 1, 2, {}
    for s in sorted(freq, key=lambda s: (freq[s], -s)):
        out[s] = a
        a, b = b, a + b
    return out


def canonical(bits, vals):
    """{symbol: (code, length)} of a DHT table."""
    out, code, p = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[p]] = (code, length)
            code += 1
            p += 1
        code <<= 1
    return out


def _dct_matrix():
    c = np.zeros((8, 8))
    for u in range(8):
        for x in range(8):
            c[u, x] = (np.sqrt(0.125) if u == 0 else 0.5) * np.cos((2 * x + 1) * u * np.pi / 16)
    return c


_C = _dct_matrix()


def planes(a, layout, rgb=False):
    """Component planes (float samples), each padded to whole MCUs by edge replication and box-downsampled for chroma."""
    a = np.asarray(a)
    if a.ndim == 2:
        a = np.repeat(a[:, :, None], 3, 2)
    h, w = a.shape[:2]
    hs, vs = SAMPLING[layout]
    mh, mw = 8 * vs, 8 * hs
    H, W = -(-h // mh) * mh, -(-w // mw) * mw
    f = a.astype(np.float64)
    if layout == "gray":
        comps = [f[:, :, 0]]
    elif rgb:
        comps = [f[:, :, 0], f[:, :, 1], f[:, :, 2]]
    else:
        r, g, b = f[:, :, 0], f[:, :, 1], f[:, :, 2]
        comps = [0.299 * r + 0.587 * g + 0.114 * b, -0.168736 * r - 0.331264 * g + 0.5 * b + 128,
                 0.5 * r - 0.418688 * g - 0.081312 * b + 128]
        comps = [np.clip(np.round(c), 0, 255) for c in comps]
    comps = [np.pad(c, ((0, H - h), (0, W - w)), mode="edge") for c in comps]
    for k in (1, 2):
        if k < len(comps) and (hs, vs) != (1, 1):
            c = comps[k]
            comps[k] = c.reshape(H // vs, vs, W // hs, hs).mean(axis=(1, 3))
    return comps


def quantise(plane, qzz):
    """[by, bx, 64] int coefficients in zig-zag order of one plane (float DCT, rounding quantisation, clamped to |value| <= 1023)."""
    hb, wb = plane.shape[0] // 8, plane.shape[1] // 8
    blocks = plane.reshape(hb, 8, wb, 8).transpose(0, 2, 1, 3) - 128.0
    coef = np.einsum("ux,abxy,vy->abuv", _C, blocks, _C).reshape(hb, wb, 64)[:, :, ZIGZAG]
    q = np.asarray(qzz, np.float64)
    qc = np.round(coef / q)
    lim = np.floor(1023.0 / q)
    return np.clip(qc, -lim, lim).astype(np.int64)


def _cat(v):
    return 0 if v == 0 else int(abs(v)).bit_length()


def _bits(v, s):
    return v if v >= 0 else v + (1 << s) - 1


def _segment_bytes(bits):
    """A bit string -> padded with 1-bits to a byte, byte-stuffed."""
    if not bits:
        return b""
    bits += "1" * (-len(bits) % 8)
    raw = int(bits, 2).to_bytes(len(bits) // 8, "big")
    return raw.replace(b"\xff", b"\xff\x00")


def encode(a, layout="420", quality=75, *, rgb=False, ids=None, markers=(("jfif", 16),), qidx=None, q16=False, qtables=None,
           dcidx=None, acidx=None, huff="std", dht="split", redefine=False, ri=0, fill=0, eoi_fill=None, extra=(), trailing=b"",
           drop_rst=None, extra_rst=None, zrl_past_63=None):
    """JPEG bytes of `a` (uint8 [h, w, 3], or [h, w] / channel 0 for gray).

    rgb: store R, G, B unconverted (else YCbCr).  ids: component IDs (default 1, 2, 3).  markers: colour signalling in order, each
    ('jfif', segment length) or ('adobe', transform).  qidx / dcidx / acidx: table index per component (default 0, 1, 1).  q16: 16-bit
    DQT and SOF1.  qtables: {index: 64 zig-zag values} to use instead of the scaled Annex K tables.  huff: 'std' (Annex K), 'opt' (K.2 from
    the data's counts) or 'deep' (K.2 from Fibonacci-ranked counts: 16-bit codes).  dht: 'split' (one segment per table) or 'merged'.
    redefine: every table is first defined with other contents, then redefined right before SOS.  ri: restart interval in MCUs; fill /
    eoi_fill: 0xFF fill bytes before each RSTn / before EOI.  extra: (marker, payload) segments after SOI.  trailing: bytes after EOI.
    Corruption: drop_rst / extra_rst: the RSTn after interval j left out / written twice; zrl_past_63: in that block, after the DC,
    three ZRLs and a (15, 1) symbol (coefficient index 64)."""
    a = np.asarray(a)
    h, w = a.shape[:2]
    std = standard_tables()
    nc = 1 if layout == "gray" else 3
    hs, vs = SAMPLING[layout]
    samp = [(hs, vs)] + [(1, 1)] * (nc - 1)
    ids = list(ids or [1, 2, 3])[:nc]
    qidx = list(qidx or [0, 1, 1])[:nc]
    dcidx = list(dcidx or [0, 1, 1])[:nc]
    acidx = list(acidx or [0, 1, 1])[:nc]

    def first_user(idxs, t):                                         # luma contents if component 0 is the first to use table t
        return 0 if idxs.index(t) == 0 else 1
    qt = dict(qtables or {})
    for t in qidx:
        if t not in qt:
            qt[t] = scaled_qtable(std["q"][first_user(qidx, t)], quality)
    ps = planes(a, layout, rgb)
    co = [quantise(p, qt[qidx[c]]) for c, p in enumerate(ps)]

    # symbols: per restart interval, a list of (component, is_ac, symbol, extra bits, extra length)
    if nc == 1:
        mcuy, mcux = co[0].shape[:2]
    else:
        mcux, mcuy = -(-w // (8 * hs)), -(-h // (8 * vs))
    nmcu = mcux * mcuy
    intervals, cur, pred, blk_no = [], [], [0] * nc, 0
    for m in range(nmcu):
        if ri and m and m % ri == 0:
            intervals.append(cur)
            cur, pred = [], [0] * nc
        my, mx = divmod(m, mcux)
        for c in range(nc):
            ch, cv = samp[c]
            for y in range(cv):
                for x in range(ch):
                    blk = co[c][my * cv + y, mx * ch + x].tolist()
                    d = blk[0] - pred[c]
                    pred[c] = blk[0]
                    s = _cat(d)
                    cur.append((c, 0, s, _bits(d, s), s))
                    if blk_no == zrl_past_63:
                        cur += [(c, 1, 0xF0, 0, 0)] * 3 + [(c, 1, 0xF1, 1, 1)]
                        blk_no += 1
                        continue
                    blk_no += 1
                    run = 0
                    last = max([k for k in range(1, 64) if blk[k]] or [0])
                    for k in range(1, last + 1):
                        v = blk[k]
                        if v == 0:
                            run += 1
                            continue
                        while run > 15:
                            cur.append((c, 1, 0xF0, 0, 0))
                            run -= 16
                        s = _cat(v)
                        cur.append((c, 1, (run << 4) | s, _bits(v, s), s))
                        run = 0
                    if last < 63:
                        cur.append((c, 1, 0x00, 0, 0))
    intervals.append(cur)

    # Huffman tables per (class, index)
    used = sorted({(0, dcidx[c]) for c in range(nc)} | {(1, acidx[c]) for c in range(nc)})
    tabs = {}
    for tc, th in used:
        idxs = dcidx if tc == 0 else acidx
        if huff == "std":
            tabs[(tc, th)] = std["ac" if tc else "dc"][first_user(idxs, th)]
        else:
            freq = {}
            for iv in intervals:
                for c, is_ac, sym, _, _ in iv:
                    if is_ac == tc and idxs[c] == th:
                        freq[sym] = freq.get(sym, 0) + 1
            tabs[(tc, th)] = optimal_table(fib_ranked(freq) if huff == "deep" else freq)
    codes = {k: canonical(*v) for k, v in tabs.items()}

    out = bytearray(b"\xff\xd8")

    def seg(marker, payload):
        out.extend(bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload))
    for m, payload in extra:
        seg(m, payload)
    for kind, v in markers:
        if kind == "jfif":
            full = b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"
            seg(0xE0, (full + b"\x00" * max(0, v - 16))[:v - 2])
        else:
            seg(0xEE, b"Adobe\x00\x64\x00\x00\x00\x00" + bytes([v]))

    def dht_payload(tc, th, table):
        bits, vals = table
        return bytes([(tc << 4) | th] + list(bits) + list(vals))
    if redefine:                                                     # other (valid) contents under the same indices first
        for tc, th in used:
            alt = std["ac" if tc else "dc"][1 - first_user(dcidx if tc == 0 else acidx, th)]
            seg(0xC4, dht_payload(tc, th, alt))
    qpay = b""
    for t in sorted(qt):
        if t in qidx:
            vals = qt[t]
            qpay += bytes([(16 if q16 else 0) | t]) + (b"".join(int(v).to_bytes(2, "big") for v in vals) if q16 else bytes(vals))
    seg(0xDB, qpay)
    sof = bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([nc])
    for c in range(nc):
        sof += bytes([ids[c], (samp[c][0] << 4) | samp[c][1], qidx[c]])
    seg(0xC1 if q16 else 0xC0, sof)
    pays = [dht_payload(tc, th, tabs[(tc, th)]) for tc, th in used]
    if dht == "merged":
        seg(0xC4, b"".join(pays))
    else:
        for p in pays:
            seg(0xC4, p)
    if ri:
        seg(0xDD, ri.to_bytes(2, "big"))
    sos = bytes([nc])
    for c in range(nc):
        sos += bytes([ids[c], (dcidx[c] << 4) | acidx[c]])
    seg(0xDA, sos + b"\x00\x3f\x00")

    table_of = [(codes[(0, dcidx[c])], codes[(1, acidx[c])]) for c in range(nc)]
    for j, iv in enumerate(intervals):
        parts = []
        for c, is_ac, sym, val, n in iv:
            code, ln = table_of[c][is_ac][sym]
            parts.append(format(code, "0%db" % ln))
            if n:
                parts.append(format(val, "0%db" % n))
        out.extend(_segment_bytes("".join(parts)))
        if j + 1 < len(intervals):
            mk = b"\xff" * fill + bytes([0xFF, 0xD0 + j % 8])
            if j == drop_rst:
                mk = b""
            elif j == extra_rst:
                mk = mk + bytes([0xFF, 0xD0 + (j + 1) % 8])
            out.extend(mk)
    out.extend(b"\xff" * (fill if eoi_fill is None else eoi_fill) + b"\xff\xd9" + trailing)
    return bytes(out)


def mcu_counts(w, h, layout):
    """(mcux, mcuy) of a frame."""
    hs, vs = SAMPLING[layout]
    if layout == "gray":
        return -(-w // 8), -(-h // 8)
    return -(-w // (8 * hs)), -(-h // (8 * vs))


# ------------------------------------------------------------------------------------------------ test contents
def _smooth(w, h):
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([x * 255 // max(w - 1, 1), y * 255 // max(h - 1, 1), (x + y) * 127 // max(w + h - 2, 1)], 2).astype(np.uint8)


def textured(w, h, seed):
    """Gradients plus mild noise: content a quality-75 encode keeps above 30 dB."""
    rng = np.random.default_rng(seed)
    a = _smooth(w, h).astype(np.int64) + rng.integers(-12, 13, (h, w, 3))
    return np.clip(a, 0, 255).astype(np.uint8)


RGB_IDS, YCC_IDS = [82, 71, 66], [1, 2, 3]
GUESS_CASES = ([((), ids) for ids in (RGB_IDS, YCC_IDS, [0, 1, 2], [82, 71, 67], [114, 103, 98])]
               + [((("jfif", 16),), ids) for ids in (RGB_IDS, YCC_IDS)]
               + [((("jfif", 16), ("adobe", 0)), RGB_IDS), ((("adobe", 0), ("jfif", 16)), YCC_IDS)]
               + [((("jfif", n), ("adobe", 0)), ids) for n in range(9, 16) for ids in (RGB_IDS, YCC_IDS)]
               + [((("jfif", n),), ids) for n in (9, 12, 15) for ids in (RGB_IDS, YCC_IDS)]
               + [((("adobe", t),), ids) for t in (0, 1, 2) for ids in (RGB_IDS, YCC_IDS, [5, 6, 7])])


def colour_case(markers, ids, layout="444", w=40, h=24):
    """The source and a file whose components hold R, G, B unconverted, signalled by `markers` and `ids`."""
    a = _smooth(w, h)
    return a, encode(a, layout, 100, rgb=True, ids=ids, markers=markers)
