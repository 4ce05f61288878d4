"""What `Image.save(f, "JPEG", quality=q[, subsampling=s])` writes, restated in numpy integer arithmetic (test infrastructure): the
reference for csrc/yf_jpeg_enc_kernels.hip wherever PIL itself is not at hand.  tests/test_cpu_jpeg_enc.py holds it to PIL's bytes.

`encode(a, quality, subsampling)`: `a` uint8 [h, w, 3] RGB or [h, w] gray -> the complete file bytes.

  header     SOI, JFIF 1.01 APP0 (density 1 x 1, no unit), one DQT segment per table (zig-zag order), SOF0 (components 1, 2, 3; luma
             sampling from `subsampling`, chroma 1 x 1 on table 1), one DHT segment per Annex K table in the order DC 0, AC 0, DC 1, AC 1
             (gray: the first two), SOS.  No restart interval, no comment.
  tables     Annex K.1 scaled by libjpeg's jpeg_quality_scaling, clamped to 1..255 (tests/jpeg_write.py:scaled_qtable)
  colour     rgb_ycc_convert: 16-bit fixed-point tables, Cb / Cr with the 128 offset and ONE_HALF - 1
  sampling   the luma plane is replicated to whole 8 x 8 blocks.  Chroma: the input columns are replicated to twice (4:2:0, 4:2:2) the
             chroma plane's block-padded width and the input rows to an even count (4:2:0) BEFORE the 2 x 2 (bias 1, 2, 1, ...) or
             2 x 1 (bias 0, 1, 0, ...) mean; the downsampled rows are replicated to whole blocks AFTER it (jcprepct.c pads the
             conversion buffer to one row group and then the downsampled output to the iMCU height)
  blocks     a luma block of an MCU that lies wholly right of or below the luma plane's own blocks is no picture data: libjpeg
             (jccoefct.c) codes it as zeros with the quantised DC of the block before it (right edge), or of the last block of the row
             of blocks above it in that MCU (bottom edge)
  DCT        jfdctint.c (CONST_BITS 13, PASS1_BITS 2, samples level-shifted by 128, output scaled by 8), quantised against 8 * q:
             (|v| + 4 * q) // (8 * q) with the sign put back
  entropy    Annex K Huffman tables: DC difference per component, (run, size) with ZRL and EOB, 0xFF 0x00 stuffing, the last byte
             padded with one-bits, EOI"""
import numpy as np

from jpeg_write import ZIGZAG, scaled_qtable, standard_tables

SUBSAMPLING = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2), 0: (1, 1), 1: (2, 1), 2: (2, 2)}     # luma (h, v)

F_0_298, F_0_390, F_0_541, F_0_765, F_0_899, F_1_175 = 2446, 3196, 4433, 6270, 7373, 9633
F_1_501, F_1_847, F_1_961, F_2_053, F_2_562, F_3_072 = 12299, 15137, 16069, 16819, 20995, 25172


def qtables(quality):
    """[luma, chroma] in zig-zag order."""
    return [scaled_qtable(t, quality) for t in standard_tables()["q"]]


def _seg(marker, payload):
    return bytes([0xFF, marker, (len(payload) + 2) >> 8, (len(payload) + 2) & 255]) + bytes(payload)


def header(h, w, ncomp, quality, hs=2, vs=2):
    std, q = standard_tables(), qtables(quality)
    out = b"\xff\xd8" + _seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for t in range(2 if ncomp == 3 else 1):
        out += _seg(0xDB, [t] + q[t])
    sof = [8, h >> 8, h & 255, w >> 8, w & 255, ncomp]
    for c in range(ncomp):
        sof += [c + 1, (hs << 4 | vs) if (c == 0 and ncomp == 3) else 0x11, min(c, 1)]
    out += _seg(0xC0, sof)
    for t in range(2 if ncomp == 3 else 1):
        for cls, key in ((0, "dc"), (1, "ac")):
            bits, vals = std[key][t]
            out += _seg(0xC4, [cls << 4 | t] + list(bits) + list(vals))
    sos = [ncomp]
    for c in range(ncomp):
        sos += [c + 1, 0x11 * min(c, 1)]
    return out + _seg(0xDA, sos + [0, 63, 0])


def rgb_to_ycc(a):
    r, g, b = (a[..., i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _pad(p, rows, cols):
    return np.pad(p, ((0, rows - p.shape[0]), (0, cols - p.shape[1])), mode="edge")


def _ceil(a, b):
    return -(-a // b)


def planes(a, hs, vs):
    """[(plane padded to its own whole blocks, h_samp, v_samp)] per component."""
    if a.ndim == 2:
        h, w = a.shape
        return [(_pad(a.astype(np.int64), _ceil(h, 8) * 8, _ceil(w, 8) * 8), 1, 1)]
    h, w = a.shape[:2]
    y, cb, cr = rgb_to_ycc(a)
    out = [(_pad(y, _ceil(h, 8) * 8, _ceil(w, 8) * 8), hs, vs)]
    cw, ch = _ceil(w, hs), _ceil(h, vs)
    cwp, chp = _ceil(cw, 8) * 8, _ceil(ch, 8) * 8
    for c in (cb, cr):
        c = _pad(c, ch * vs, cwp * hs)
        if (hs, vs) == (2, 2):
            bias = 1 + (np.arange(cwp) & 1)
            c = (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + bias) >> 2
        elif (hs, vs) == (2, 1):
            c = (c[:, 0::2] + c[:, 1::2] + (np.arange(cwp) & 1)) >> 1
        out.append((_pad(c, chp, cwp), 1, 1))
    return out


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _pass(d, first):
    """One jfdctint pass along the last axis of d [..., 8]."""
    t0, t7, t1, t6 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7], d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5, t3, t4 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5], d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o = np.empty_like(d)
    n = 13 - 2 if first else 13 + 2
    if first:
        o[..., 0], o[..., 4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        o[..., 0], o[..., 4] = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
    z1 = (t12 + t13) * F_0_541
    o[..., 2] = _descale(z1 + t13 * F_0_765, n)
    o[..., 6] = _descale(z1 - t12 * F_1_847, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * F_1_175
    t4, t5, t6, t7 = t4 * F_0_298, t5 * F_2_053, t6 * F_3_072, t7 * F_1_501
    z1, z2, z3, z4 = -z1 * F_0_899, -z2 * F_2_562, -z3 * F_1_961 + z5, -z4 * F_0_390 + z5
    o[..., 7], o[..., 5] = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n)
    o[..., 3], o[..., 1] = _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return o


def fdct_quant(plane, qzz):
    """plane [8R, 8C] -> quantised coefficients [R, C, 64] in zig-zag order."""
    R, C = plane.shape[0] // 8, plane.shape[1] // 8
    b = plane.reshape(R, 8, C, 8).transpose(0, 2, 1, 3) - 128
    b = _pass(b, True)
    b = _pass(b.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)
    nat = np.empty(64, np.int64)
    nat[ZIGZAG] = np.asarray(qzz, np.int64) * 8
    b = b.reshape(R, C, 64)
    qv = (np.abs(b) + (nat >> 1)) // nat
    return (np.sign(b) * qv)[..., ZIGZAG]


def scan_blocks(a, quality, hs, vs):
    """(coefficients [blocks, 64] zig-zag in scan order, component index per block)."""
    q = qtables(quality)
    comps = planes(a, hs, vs)
    h, w = a.shape[:2]
    if len(comps) == 1:
        co = fdct_quant(comps[0][0], q[0])
        return co.reshape(-1, 64), np.zeros(co.shape[0] * co.shape[1], np.int64)
    mr, mc = _ceil(h, 8 * vs), _ceil(w, 8 * hs)
    per = []
    for ci, (p, chs, cvs) in enumerate(comps):
        co = fdct_quant(p, q[min(ci, 1)])
        R, C = co.shape[:2]
        full = np.zeros((mr * cvs, mc * chs, 64), np.int64)
        full[:R, :C] = co
        if C < mc * chs:                                  # dummy blocks at the right edge: the DC of the block before
            full[:R, C, 0] = full[:R, C - 1, 0]
        if R < mr * cvs:                                  # a dummy row at the bottom: the DC of the MCU's last block in the row above
            full[R, :, 0] = np.repeat(full[R - 1, chs - 1::chs, 0], chs)
        per.append(full.reshape(mr, cvs, mc, chs, 64).transpose(0, 2, 1, 3, 4).reshape(mr, mc, cvs * chs, 64))
    blocks = np.concatenate(per, axis=2)
    comp = np.concatenate([np.full(p.shape[2], i) for i, p in enumerate(per)])
    return blocks.reshape(-1, 64), np.tile(comp, mr * mc)


def huff_codes(bits, vals):
    """(code, size) arrays indexed by symbol (jpeg_make_c_derived_tbl)."""
    code, size = np.zeros(256, np.int64), np.zeros(256, np.int64)
    c, k = 0, 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            code[vals[k]], size[vals[k]] = c, l
            c += 1
            k += 1
        c <<= 1
    return code, size


def _nbits(v):
    v = np.abs(v)
    n = np.zeros(v.shape, np.int64)
    for i in range(12):
        n += (v >> i) > 0
    return n


def entropy(blocks, comp):
    """The entropy-coded segment (stuffed, padded) of blocks [B, 64] whose component indices are `comp`."""
    std = standard_tables()
    B = blocks.shape[0]
    tab = np.minimum(comp, 1)
    dc = blocks[:, 0]
    diff = dc.copy()
    for c in np.unique(comp):
        i = np.nonzero(comp == c)[0]
        diff[i] = np.diff(dc[i], prepend=0)
    keys, vals, lens = [], [], []

    def emit(key, t, sym, extra, nextra, kind):
        for tt in (0, 1):
            m = t == tt
            code, size = huff_codes(*std[kind][tt])
            assert np.all(size[sym[m]] > 0)
            keys.append(key[m])
            vals.append(code[sym[m]] << nextra[m] | extra[m])
            lens.append(size[sym[m]] + nextra[m])

    blk = np.arange(B)
    n = _nbits(diff)
    emit(blk * 256, tab, n, np.where(diff < 0, diff - 1, diff) & ((1 << n) - 1), n, "dc")
    bi, k = np.nonzero(blocks[:, 1:])
    k = k + 1
    v = blocks[bi, k]
    prev = np.where(np.diff(bi, prepend=-1) != 0, 0, np.concatenate([[0], k[:-1]]))
    run = k - prev - 1
    zero = np.zeros(len(bi), np.int64)
    for j in range(3):
        m = run >= 16 * (j + 1)
        emit((bi * 256 + k * 4 + j)[m], tab[bi][m], np.full(m.sum(), 0xF0), zero[m], zero[m], "ac")
    n = _nbits(v)
    emit(bi * 256 + k * 4 + 3, tab[bi], (run & 15) << 4 | n, np.where(v < 0, v - 1, v) & ((1 << n) - 1), n, "ac")
    eob = blocks[:, 63] == 0
    emit((blk * 256 + 255)[eob], tab[eob], np.zeros(eob.sum(), np.int64), np.zeros(eob.sum(), np.int64), np.zeros(eob.sum(), np.int64), "ac")
    keys, vals, lens = np.concatenate(keys), np.concatenate(vals), np.concatenate(lens)
    o = np.argsort(keys, kind="stable")
    vals, lens = vals[o].astype(np.uint64), lens[o]
    off = np.concatenate([[0], np.cumsum(lens)])
    total = int(off[-1])
    words = np.zeros(total // 32 + 2, np.uint64)
    win = vals << (64 - (off[:-1] & 31) - lens).astype(np.uint64)
    np.bitwise_or.at(words, off[:-1] >> 5, win >> np.uint64(32))
    np.bitwise_or.at(words, (off[:-1] >> 5) + 1, win & np.uint64(0xFFFFFFFF))
    by = words.astype(">u4").view(np.uint8)[:(total + 7) // 8].copy()
    if total & 7:
        by[-1] |= (1 << (8 - (total & 7))) - 1
    ff = np.nonzero(by == 0xFF)[0]
    return np.insert(by, ff + 1, 0).tobytes()


def encode(a, quality=75, subsampling="4:2:0"):
    a = np.asarray(a)
    assert a.dtype == np.uint8 and (a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 3))
    hs, vs = SUBSAMPLING[subsampling] if a.ndim == 3 else (1, 1)
    h, w = a.shape[:2]
    blocks, comp = scan_blocks(a, quality, hs, vs)
    return header(h, w, 3 if a.ndim == 3 else 1, quality, hs, vs) + entropy(blocks, comp) + b"\xff\xd9"
