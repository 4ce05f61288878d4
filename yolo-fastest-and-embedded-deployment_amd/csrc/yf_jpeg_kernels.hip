// yf_jpeg_kernels.hip -- baseline and, opt-in, progressive JPEG decoding on the device, bit for bit what PIL (libjpeg-turbo with its defaults: ISLOW integer IDCT,
// fancy upsampling, integer YCbCr->RGB tables) returns, as cv2.imread's BGR bytes [n, h, w, 3].
//   host (yf_jpeg_pack): marker parsing of n files of one size, refusal of everything outside the supported subset (progressive, lossless,
//     arithmetic, 12-bit, 2 or >= 4 components, other sampling layouts, several scans, DNL), Huffman tables as a 9-bit lookahead table plus
//     libjpeg's maxcode / valoffset for longer codes, quantisation tables in natural order, component geometry, and one blob holding the
//     descriptors, tables and raw entropy-coded bytes of every frame.  No GPU call.
//   jpeg_entropy_kernel: one wave per frame.  (1) The 64 lanes remove byte stuffing and find RSTn markers 64 bytes at a time (ballot +
//     popcount prefix) into a clean bit stream and a table of interval starts.  (2) The scan is cut into 64 stretches: at interval starts
//     when the file has restart markers (each lane owns whole intervals, its start state is exact), otherwise into 64 equal runs of bits
//     (Weissenberger & Schmidt, HiPC 2021): every lane decodes its run from a guessed state (block 0 of an MCU, DC next), stopping at the
//     first symbol boundary at or past the next lane's start; a lane whose start state differs from its left neighbour's end state decodes
//     again from that state, until no start state changes.  Huffman codes self-synchronise, so a redone lane usually ends where it ended
//     before and the chain of changes stops after one round; it cannot take more than 64 rounds (after round r, lanes 0..r are exact).
//     Correctness never depends on synchronisation.  (3) A wave prefix over the MCUs each lane completed and its per-component DC
//     differences gives every lane its first MCU and DC predictors, and (4) one more pass writes the int16 coefficients in natural order.
//   jpeg_idct_kernel: dequantise + libjpeg's jpeg_idct_islow (CONST_BITS 13, PASS1_BITS 2, 64-bit intermediates as JLONG, the post-IDCT
//     range-limit table with its `& 0x3FF` wrap), one thread per 8x8 block, into one uint8 plane per component.
//   jpeg_color_kernel: libjpeg-turbo's fancy upsampling (h2v1: triangle filter with biases 1 / 2; h1v2: vertical filter with biases 1 / 2;
//     h2v2: vertical 3:1 then horizontal with biases 8 / 7; plain replication for h2v1 / h2v2 when the chroma is <= 2 samples wide, as
//     jinit_upsampler chooses; edges replicate the last real row / column), ycc_rgb_convert's integer tables (SCALEBITS 16), BGR stores of
//     4 pixels (three 4-byte words) per thread.
//   progressive files (yf_jpeg_pack_ex with YF_JPEG_PROGRESSIVE): the host parses every scan (tables snapshot per scan, quantisation
//     tables latched at a component's first scan as libjpeg does), checks the scan script (a malformed or incomplete progression is
//     refused: libjpeg smooths blocks of unknown accuracy) and sorts the scans by dependency level.  jpeg_prog_entropy_kernel decodes
//     them, one workgroup per frame and one wave per scan of a level, into the same coefficient blocks; IDCT and colour are shared.
// Corrupt entropy data: reads stay inside the frame's clean stream (zero bits past its end, as libjpeg pads), coefficient indices are
// clamped, writes stay in the frame's planes; the frame's status word gets a flag (bad Huffman code, coefficient index past 63, data
// exhausted before the last MCU, restart markers missing or extra).
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/yolo_fastest_hip.h"

namespace yf {
int set_error(int code, const char* msg);   // yf_engine.hip: the slot yf_last_error_string() reads
}

namespace {

int fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return yf::set_error(code, buf);
}
#define HIP_OK(expr)                                                                                     \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess) return fail(YF_E_HIP, "%s failed: %s", #expr, hipGetErrorString(e_));      \
    } while (0)

constexpr uint32_t JPG_MAGIC = 0x3147504Au;       // "JPG1"
constexpr int JPG_LANES = 64;                     // one wave per frame
constexpr int JPG_MAX_BPM = 6;                    // blocks per MCU: 4 luma + 2 chroma at most
constexpr int JPG_MAX_DIM = 8192;
constexpr uint32_t JPG_MAX_DATA = 1u << 28;       // entropy bytes per frame: bit positions stay in uint32

// status flags (yf_jpeg_decode_u8's d_status)
constexpr int ST_BAD_CODE = 1, ST_BAD_INDEX = 2, ST_TRUNCATED = 4, ST_RESTART = 8;

struct JHuff {                   // one Huffman table
    uint16_t lut[512];           // 9-bit lookahead: (length << 8) | symbol; length 0 = the code is longer than 9 bits
    int32_t maxcode[18];         // libjpeg's jpeg_make_d_derived_tbl: largest code of length l (-1: none)
    int32_t valoffset[18];       // symbol index = code + valoffset[l]
    uint8_t huffval[256];
};
struct JTables {
    JHuff huff[8];               // DC 0..3, AC 0..3
    uint16_t q[4][64];           // natural order
};
struct JComp {
    int h, v;                    // sampling factors (1 x 1 for a one-component frame)
    int bw, bh;                  // blocks per row / column of the MCU-padded plane
    int dw, dh;                  // downsampled_width / _height: ceil(w * h / hmax), ceil(h * v / vmax)
    int q, dc, ac;               // table indices
    int blk0;                    // first block of this component in the frame's coefficient run
    uint64_t plane_off;          // workspace byte offset of the uint8 plane [bh * 8][bw * 8]
};
struct JFrame {
    uint64_t data_off;           // blob byte offset of the entropy-coded bytes
    uint32_t data_len;
    int ncomp, color;            // color: 0 gray, 1 YCbCr, 2 RGB
    int mcux, mcuy, nmcu, bpm;   // MCUs per row / column, MCUs, blocks per MCU
    int ri, nint;                // restart interval (MCUs, 0 = none), intervals (1 without restarts)
    int nblocks;
    int8_t bcomp[JPG_MAX_BPM], bx[JPG_MAX_BPM], by[JPG_MAX_BPM];
    int8_t prog;                 // 1: a progressive frame (its scans are in the blob's JProg section; jpeg_prog_entropy_kernel decodes it)
    int8_t pad_[5];
    JComp comp[3];
    uint64_t tables_off;         // blob byte offset of this frame's JTables
    uint64_t clean_off;          // workspace: clean stream (clean_cap bytes), interval starts int32 [nint + 1], coefficients int16
    uint64_t clean_cap, istart_off, coef_off;
};
struct JHeader {
    uint32_t magic;
    int n, h, w;
    uint64_t blob_bytes, ws_bytes;
    uint64_t coef_begin, coef_end;   // workspace span of all coefficient runs (zeroed before the entropy pass)
    int max_blocks, pad_;
    int version, nprog;              // blob format; progressive frames in the blob (0: the blob has no JProg section)
    uint64_t prog_off;               // blob byte offset of JProg[n]
};
struct JScan {                   // one scan of a progressive frame (ITU-T T.81 Annex G); a frame's scans are sorted by (level, index)
    uint64_t data_off;           // blob byte offset of the scan's entropy-coded bytes
    uint32_t data_len, file_off; // their length, and their offset in the file
    int index, level;            // position in the file; dependency level (scans of one level write disjoint coefficients)
    int ncomp, comp[3];          // components in scan order
    int tab[3], tid[3];          // per scan component: index into the frame's JHuff snapshots (-1: none), the table id it was named by
    int ss, se, ah, al;
    int ri, nint;                // restart interval in this scan's MCUs (0 = none), intervals
    int nmcu, mcux, bpm;         // this scan's MCUs (non-interleaved: the component's real blocks, one per MCU), MCUs per row, blocks per MCU
    int8_t bcomp[JPG_MAX_BPM], bx[JPG_MAX_BPM], by[JPG_MAX_BPM];   // bcomp: position in comp[]
    int8_t pad_[2];
    uint64_t clean_off, clean_cap, istart_off;   // workspace: clean stream, interval starts int32 [nint + 1]
};
struct JProg {                   // per frame of a blob with progressive frames (zeros for a baseline frame)
    uint64_t scans_off, huff_off;   // blob byte offsets of JScan[nscan] and of the JHuff snapshots
    int nscan, nlevel, nhuff, pad_;
};
constexpr int JPG_VERSION = 2;
constexpr int JPG_MAX_SCANS = 256;
constexpr int JPG_PROG_WAVES = 8;                 // waves per workgroup of jpeg_prog_entropy_kernel: scans of one level decoded at a time

__host__ __device__ inline uint64_t align_up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }

// zig-zag position -> natural position
__constant__ uint8_t c_natural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                      41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                      30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
const uint8_t h_natural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                               41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                               30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// ---------------------------------------------------------------------------------------------------------------- host: parsing
struct Parsed {
    const uint8_t* data = nullptr;
    uint32_t data_len = 0;
    int h = 0, w = 0;
    JFrame f{};
    JTables t{};
    // progressive files (f.prog): the scans in file order with their bytes, and the Huffman table snapshots they name
    std::vector<JScan> scans;
    std::vector<const uint8_t*> sdata;
    std::vector<JHuff> huffs;
    int nlevel = 0;
};

struct Reader {
    const uint8_t* p;
    size_t n, i;
    bool has(size_t k) const { return i + k <= n; }
    int u8() { return p[i++]; }
    int u16() { int v = (p[i] << 8) | p[i + 1]; i += 2; return v; }
};

// libjpeg's jpeg_make_d_derived_tbl; false on a malformed table
bool build_huff(const uint8_t bits[17], const uint8_t* vals, int nvals, bool dc, JHuff& t)
{
    memset(&t, 0, sizeof t);
    memcpy(t.huffval, vals, nvals);
    int huffsize[257], huffcode[257], p = 0;
    for (int l = 1; l <= 16; ++l)
        for (int i = 0; i < bits[l]; ++i) huffsize[p++] = l;
    huffsize[p] = 0;
    const int numsymbols = p;
    int code = 0, si = huffsize[0];
    p = 0;
    while (huffsize[p]) {
        while (huffsize[p] == si) huffcode[p++] = code++;
        if (code >= (1 << si)) return false;
        code <<= 1;
        si++;
    }
    p = 0;
    for (int l = 1; l <= 16; ++l) {
        if (bits[l]) {
            t.valoffset[l] = p - huffcode[p];
            p += bits[l];
            t.maxcode[l] = huffcode[p - 1];
        } else {
            t.maxcode[l] = -1;
        }
    }
    t.valoffset[17] = 0;
    t.maxcode[17] = 0xFFFFF;
    p = 0;
    for (int l = 1; l <= 9; ++l)
        for (int i = 0; i < bits[l]; ++i, ++p) {
            const int base = huffcode[p] << (9 - l);
            for (int f = 0; f < (1 << (9 - l)); ++f) t.lut[base | f] = (uint16_t)((l << 8) | vals[p]);
        }
    if (dc)
        for (int i = 0; i < numsymbols; ++i)
            if (vals[i] > 15) return false;
    return true;
}

// Geometry of a frame whose components are sampled (ch, cv): MCU counts, per-component block counts and sizes, first blocks.
void frame_geometry(JFrame& f, int nf, const int* ch, const int* cv, int H, int W)
{
    f.ncomp = nf;
    if (nf == 1) {
        f.comp[0].h = f.comp[0].v = 1;
        f.mcux = (W + 7) / 8;
        f.mcuy = (H + 7) / 8;
        f.comp[0].bw = f.mcux; f.comp[0].bh = f.mcuy; f.comp[0].dw = W; f.comp[0].dh = H;
    } else {
        const int hmax = ch[0], vmax = cv[0];
        f.mcux = (W + 8 * hmax - 1) / (8 * hmax);
        f.mcuy = (H + 8 * vmax - 1) / (8 * vmax);
        for (int c = 0; c < nf; ++c) {
            JComp& k = f.comp[c];
            k.h = ch[c]; k.v = cv[c];
            k.bw = f.mcux * ch[c]; k.bh = f.mcuy * cv[c];
            k.dw = (int)(((long)W * ch[c] + hmax - 1) / hmax);
            k.dh = (int)(((long)H * cv[c] + vmax - 1) / vmax);
        }
    }
    f.nmcu = f.mcux * f.mcuy;
    int blk = 0;
    for (int c = 0; c < nf; ++c) { f.comp[c].blk0 = blk; blk += f.comp[c].bw * f.comp[c].bh; }
    f.nblocks = blk;
}

// The entropy-coded bytes that start at d0: up to the first marker that is neither a stuffed 0xFF00, fill, nor RSTn (or the end of a
// truncated file).  Returns the offset of that marker, or 0 for a DNL marker.
size_t entropy_end(const uint8_t* p, size_t n, size_t d0)
{
    size_t i = d0;
    while (i < n) {
        if (p[i] == 0xFF && i + 1 < n) {
            const int m = p[i + 1];
            if (m == 0x00 || (m >= 0xD0 && m <= 0xD7)) { i += 2; continue; }
            if (m == 0xFF) { i += 1; continue; }
            if (m == 0xDC) return 0;
            break;
        }
        ++i;
    }
    return i;
}

// The end of a progressive file: the progression must be complete (libjpeg smooths blocks whose coefficients are of unknown accuracy,
// and its pixels are then not the IDCT of the coefficients); dependency levels; scans sorted by level.
const char* finish_progressive(Parsed& out, int nf, const int8_t coef_al[3][64], const uint16_t latched[3][64])
{
    for (int c = 0; c < nf; ++c)
        for (int k = 0; k < 64; ++k)
            if (coef_al[c][k] != 0) return "incomplete progression (not every coefficient is coded down to Al = 0)";
    const int ns = (int)out.scans.size();
    int nlevel = 0;
    for (int s = 0; s < ns; ++s) {
        JScan& a = out.scans[s];
        int level = 0;
        for (int t = 0; t < s; ++t) {
            const JScan& b = out.scans[t];
            if (a.ss > b.se || b.ss > a.se) continue;
            bool share = false;
            for (int i = 0; i < a.ncomp; ++i)
                for (int j = 0; j < b.ncomp; ++j) share |= a.comp[i] == b.comp[j];
            if (share && b.level + 1 > level) level = b.level + 1;
        }
        a.level = level;
        if (level + 1 > nlevel) nlevel = level + 1;
    }
    out.nlevel = nlevel;
    std::vector<int> order(ns);
    for (int s = 0; s < ns; ++s) order[s] = s;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return out.scans[x].level < out.scans[y].level; });
    std::vector<JScan> sc(ns);
    std::vector<const uint8_t*> sd(ns);
    for (int s = 0; s < ns; ++s) { sc[s] = out.scans[order[s]]; sd[s] = out.sdata[order[s]]; }
    out.scans.swap(sc);
    out.sdata.swap(sd);
    for (int c = 0; c < nf; ++c) {
        memcpy(out.t.q[c], latched[c], sizeof latched[c]);
        out.f.comp[c].q = c;
    }
    return nullptr;
}

// One file -> Parsed, or an error message (the reason of the refusal).  flags: YF_JPEG_PROGRESSIVE accepts SOF2.
const char* parse_file(const uint8_t* p, size_t n, Parsed& out, int flags)
{
    Reader r{p, n, 0};
    if (!r.has(2) || r.u8() != 0xFF || r.u8() != 0xD8) return "not a JPEG file (no SOI marker)";
    bool have_sof = false, jfif = false, adobe = false;
    int adobe_transform = -1, precision = 8, nf = 0;
    int cid[4] = {0}, ch[4] = {0}, cv[4] = {0}, cq[4] = {0};
    bool have_huff[8] = {false}, have_q[4] = {false};
    int ri = 0;
    bool prog = false;
    std::vector<JHuff> hcur(8);                      // the tables as defined so far (a scan takes a snapshot)
    memset(hcur.data(), 0, sizeof(JHuff) * 8);
    uint16_t qcur[4][64] = {{0}}, latched[3][64] = {{0}};
    bool is_latched[3] = {false, false, false};
    int8_t coef_al[3][64];                           // per coefficient: the Al it was last coded at (-1: not coded yet)
    memset(coef_al, -1, sizeof coef_al);
    for (;;) {
        // next marker: 0xFF, fill bytes, code
        if (!r.has(1)) {
            if (prog && !out.scans.empty()) return finish_progressive(out, nf, coef_al, latched);   // EOI missing: libjpeg inserts one
            return "file ends before the scan (no SOS marker)";
        }
        if (r.u8() != 0xFF) return "corrupt marker structure";
        int code;
        do {
            if (!r.has(1)) return "file ends inside a marker";
            code = r.u8();
        } while (code == 0xFF);
        if (code == 0x01 || (code >= 0xD0 && code <= 0xD7)) continue;          // standalone markers
        if (code == 0xD8) return "second SOI marker before the scan";
        if (code == 0xD9) {
            if (prog && !out.scans.empty()) return finish_progressive(out, nf, coef_al, latched);
            return "EOI marker before any scan";
        }
        if (!r.has(2)) return "file ends inside a marker length";
        const int len = r.u16();
        if (len < 2 || !r.has(len - 2)) {
            static thread_local char why[80];
            if (code == 0xC0 || code == 0xC1 || (code == 0xC2 && (flags & YF_JPEG_PROGRESSIVE)))
                snprintf(why, sizeof why, "SOF%d segment runs past the end of the file", code - 0xC0);
            else snprintf(why, sizeof why, "marker 0x%02X segment runs past the end of the file", code);
            return why;
        }
        const size_t seg_end = r.i + len - 2;
        switch (code) {
        case 0xC2:
            if (!(flags & YF_JPEG_PROGRESSIVE)) return "progressive JPEG (SOF2) is not supported";
            prog = true;
            [[fallthrough]];
        case 0xC0:
        case 0xC1: {
            if (have_sof) return "more than one SOF marker";
            if (len < 8) return "SOF segment too short";
            precision = r.u8();
            out.h = r.u16();
            out.w = r.u16();
            nf = r.u8();
            if (precision != 8) return prog ? "12-bit (or other non-8-bit) progressive JPEG is not supported"
                                            : "12-bit (or other non-8-bit) precision is not supported";
            if (len != 8 + 3 * nf) return "SOF segment length does not match its component count";
            if (nf != 1 && nf != 3) return nf == 4 ? "4-component (CMYK / YCCK) files are not supported" : "only 1- or 3-component files are supported";
            for (int c = 0; c < nf; ++c) {
                cid[c] = r.u8();
                const int hv = r.u8();
                ch[c] = hv >> 4;
                cv[c] = hv & 15;
                cq[c] = r.u8();
                if (ch[c] < 1 || ch[c] > 4 || cv[c] < 1 || cv[c] > 4 || cq[c] > 3) return "bad component sampling factor or table index";
            }
            if (out.h <= 0) return "image height 0 (DNL-defined height) is not supported";
            if (out.w <= 0) return "image width 0";
            if (out.h > JPG_MAX_DIM || out.w > JPG_MAX_DIM) return "image larger than 8192 x 8192";
            have_sof = true;
            break;
        }
        case 0xC3: return "lossless JPEG (SOF3) is not supported";
        case 0xC5: case 0xC6: case 0xC7: return "hierarchical JPEG is not supported";
        case 0xC9: case 0xCA: case 0xCB: case 0xCD: case 0xCE: case 0xCF: return "arithmetic-coded JPEG is not supported";   // SOF10 among them
        case 0xCC: return "arithmetic-coded JPEG (DAC marker) is not supported";
        case 0xC4: {
            while (r.i < seg_end) {
                if (seg_end - r.i < 17) return "DHT segment too short";
                const int tcth = r.u8();
                const int tc = tcth >> 4, th = tcth & 15;
                if (tc > 1 || th > 3) return "bad DHT table class or index";
                uint8_t bits[17] = {0};
                int count = 0;
                for (int l = 1; l <= 16; ++l) count += bits[l] = (uint8_t)r.u8();
                if (count > 256 || seg_end - r.i < (size_t)count) return "bad DHT table size";
                if (!build_huff(bits, p + r.i, count, tc == 0, hcur[tc * 4 + th])) return "bad Huffman table";
                r.i += count;
                have_huff[tc * 4 + th] = true;
            }
            break;
        }
        case 0xDB: {
            while (r.i < seg_end) {
                const int pqtq = r.u8();
                const int pq = pqtq >> 4, tq = pqtq & 15;
                if (pq > 1 || tq > 3) return "bad DQT table precision or index";
                if (seg_end - r.i < (size_t)(64 * (pq + 1))) return "DQT segment too short";
                for (int k = 0; k < 64; ++k) qcur[tq][h_natural[k]] = (uint16_t)(pq ? r.u16() : r.u8());
                have_q[tq] = true;
            }
            break;
        }
        case 0xDD:
            if (len != 4) return "bad DRI segment length";
            ri = r.u16();
            break;
        case 0xDC: return "DNL marker is not supported";
        case 0xE0:
            // libjpeg's examine_app0 needs the 14 bytes of a full JFIF header; a shorter "JFIF\0" segment does not count
            if (len >= 16 && !memcmp(p + r.i, "JFIF\0", 5)) jfif = true;
            break;
        case 0xEE:
            if (len >= 14 && !memcmp(p + r.i, "Adobe", 5)) { adobe = true; adobe_transform = p[r.i + 11]; }
            break;
        case 0xDA: {
            if (!have_sof) return "SOS marker before SOF";
            const int ns = r.u8();
            if (len != 6 + 2 * ns) return "bad SOS segment length";
            JFrame& f = out.f;
            if (prog) {
                if (ns < 1 || ns > nf) return "bad SOS component count";
                if (out.scans.size() >= (size_t)JPG_MAX_SCANS) return "more than 256 scans";
                JScan sc;
                memset(&sc, 0, sizeof sc);
                sc.index = (int)out.scans.size();
                sc.ncomp = ns;
                int tdc[3], tac[3];
                for (int s = 0; s < ns; ++s) {
                    const int cs = r.u8(), tdta = r.u8();
                    int c = -1;
                    for (int k = 0; k < nf; ++k)
                        if (cid[k] == cs) c = k;
                    if (c < 0) return "SOS names a component the frame does not have";
                    for (int k = 0; k < s; ++k)
                        if (sc.comp[k] == c) return "SOS names a component twice";
                    if ((tdta >> 4) > 3 || (tdta & 15) > 3) return "bad SOS table index";
                    sc.comp[s] = c;
                    tdc[s] = tdta >> 4;
                    tac[s] = 4 + (tdta & 15);
                }
                sc.ss = r.u8();
                sc.se = r.u8();
                const int ahal = r.u8();
                sc.ah = ahal >> 4;
                sc.al = ahal & 15;
                if (sc.ss == 0 && sc.se != 0) return "a DC scan (Ss = 0) with Se != 0";
                if (sc.ss > 0 && ns != 1) return "an AC scan (Ss > 0) with more than one component";
                if (sc.ss > 0 && (sc.se < sc.ss || sc.se > 63)) return "an AC scan with Se < Ss or Se > 63";
                if (sc.al > 13) return "successive approximation bit position Al > 13";
                if (sc.ah != 0 && sc.al != sc.ah - 1) return "a refinement scan with Al != Ah - 1";
                for (int s = 0; s < ns; ++s) {
                    int8_t* al = coef_al[sc.comp[s]];
                    if (sc.ss > 0 && al[0] < 0) return "an AC scan of a component whose DC has not been coded";
                    for (int k = sc.ss; k <= sc.se; ++k) {
                        if (sc.ah == 0 && al[k] >= 0) return "a first scan (Ah = 0) of coefficients already coded";
                        if (sc.ah != 0 && al[k] != sc.ah) return "a refinement scan whose Ah is not the Al its band was last coded at";
                        al[k] = (int8_t)sc.al;
                    }
                }
                if (out.scans.empty()) {
                    // the frame: colour space as libjpeg's default_decompress_parms guesses it, geometry
                    f.prog = 1;
                    if (nf == 1) f.color = 0;
                    else if (jfif) f.color = 1;
                    else if (adobe) f.color = adobe_transform == 0 ? 2 : 1;
                    else f.color = (cid[0] == 82 && cid[1] == 71 && cid[2] == 66) ? 2 : 1;
                    if (nf == 3 && (ch[1] != 1 || cv[1] != 1 || ch[2] != 1 || cv[2] != 1 || ch[0] > 2 || cv[0] > 2))
                        return "unsupported sampling layout (luma 1 or 2 in each direction, chroma 1 x 1)";
                    frame_geometry(f, nf, ch, cv, out.h, out.w);
                    int b = 0;
                    for (int c = 0; c < nf; ++c)
                        for (int y = 0; y < f.comp[c].v; ++y)
                            for (int x = 0; x < f.comp[c].h; ++x) { f.bcomp[b] = (int8_t)c; f.bx[b] = (int8_t)x; f.by[b] = (int8_t)y; ++b; }
                    f.bpm = b;
                    f.ri = 0;
                    f.nint = 1;
                }
                // libjpeg's latch_quant_tables: a component's table is fixed at the first scan that names it
                for (int s = 0; s < ns; ++s) {
                    const int c = sc.comp[s];
                    if (is_latched[c]) continue;
                    if (!have_q[cq[c]]) return "component uses a quantisation table that was never defined";
                    memcpy(latched[c], qcur[cq[c]], sizeof latched[c]);
                    is_latched[c] = true;
                }
                // table snapshots: DC first scans use DC tables, AC scans (first or refinement) an AC table, DC refinements none
                for (int s = 0; s < ns; ++s) {
                    sc.tab[s] = sc.tid[s] = -1;
                    if (sc.ss == 0 && sc.ah != 0) continue;
                    const int id = sc.ss == 0 ? tdc[s] : tac[s];
                    if (!have_huff[id]) return "scan uses a Huffman table that was never defined";
                    sc.tid[s] = id;
                    for (int k = 0; k < s; ++k)
                        if (sc.tid[k] == id) sc.tab[s] = sc.tab[k];
                    if (sc.tab[s] < 0) {
                        sc.tab[s] = (int)out.huffs.size();
                        out.huffs.push_back(hcur[id]);
                    }
                }
                // geometry of the scan
                if (ns == 1) {
                    const JComp& k = f.comp[sc.comp[0]];
                    sc.mcux = (k.dw + 7) / 8;
                    sc.nmcu = sc.mcux * ((k.dh + 7) / 8);
                    sc.bpm = 1;
                } else {
                    sc.mcux = f.mcux;
                    sc.nmcu = f.nmcu;
                    int b = 0;
                    for (int s = 0; s < ns; ++s) {
                        const JComp& k = f.comp[sc.comp[s]];
                        for (int y = 0; y < k.v; ++y)
                            for (int x = 0; x < k.h; ++x) { sc.bcomp[b] = (int8_t)s; sc.bx[b] = (int8_t)x; sc.by[b] = (int8_t)y; ++b; }
                    }
                    sc.bpm = b;
                }
                sc.ri = ri;
                sc.nint = ri ? (sc.nmcu + ri - 1) / ri : 1;
                const size_t d0 = r.i;
                const size_t i = entropy_end(p, n, d0);
                if (!i) return "DNL marker is not supported";
                if (i - d0 >= JPG_MAX_DATA) return "entropy-coded data larger than 256 MiB";
                sc.file_off = (uint32_t)d0;
                sc.data_len = (uint32_t)(i - d0);
                out.scans.push_back(sc);
                out.sdata.push_back(p + d0);
                r.i = i;
                continue;
            }
            if (ns != nf) return "the first scan does not hold every component (multi-scan sequential files are not supported)";
            for (int k = 0; k < 8; ++k) out.t.huff[k] = hcur[k];
            memcpy(out.t.q, qcur, sizeof qcur);
            int order[3];
            for (int s = 0; s < ns; ++s) {
                const int cs = r.u8(), tdta = r.u8();
                int c = -1;
                for (int k = 0; k < nf; ++k)
                    if (cid[k] == cs) c = k;
                if (c < 0) return "SOS names a component the frame does not have";
                for (int k = 0; k < s; ++k)
                    if (order[k] == c) return "SOS names a component twice";
                order[s] = c;
                f.comp[c].dc = tdta >> 4;
                f.comp[c].ac = 4 + (tdta & 15);
                if ((tdta >> 4) > 3 || (tdta & 15) > 3) return "bad SOS table index";
                if (!have_huff[f.comp[c].dc] || !have_huff[f.comp[c].ac]) return "scan uses a Huffman table that was never defined";
            }
            const int ss = r.u8(), se = r.u8(), ahal = r.u8();
            if (ss != 0 || se != 63 || ahal != 0) return "scan is not a sequential full-spectrum scan";
            for (int c = 0; c < nf; ++c) {
                if (!have_q[cq[c]]) return "component uses a quantisation table that was never defined";
                f.comp[c].q = cq[c];
            }
            // colour space: libjpeg's default_decompress_parms
            if (nf == 1) {
                f.color = 0;
            } else if (jfif) {
                f.color = 1;
            } else if (adobe) {
                f.color = adobe_transform == 0 ? 2 : 1;
            } else {
                f.color = (cid[0] == 82 && cid[1] == 71 && cid[2] == 66) ? 2 : 1;
            }
            // geometry
            if (nf == 3 && (ch[1] != 1 || cv[1] != 1 || ch[2] != 1 || cv[2] != 1 || ch[0] > 2 || cv[0] > 2))
                return "unsupported sampling layout (luma 1 or 2 in each direction, chroma 1 x 1)";
            frame_geometry(f, nf, ch, cv, out.h, out.w);
            if (nf == 1) {
                f.bpm = 1;
                f.bcomp[0] = 0; f.bx[0] = 0; f.by[0] = 0;
            } else {
                int b = 0;
                for (int s = 0; s < ns; ++s) {
                    const int c = order[s];
                    for (int y = 0; y < cv[c]; ++y)
                        for (int x = 0; x < ch[c]; ++x) { f.bcomp[b] = (int8_t)c; f.bx[b] = (int8_t)x; f.by[b] = (int8_t)y; ++b; }
                }
                f.bpm = b;
            }
            f.ri = ri;
            f.nint = ri ? (f.nmcu + ri - 1) / ri : 1;
            // entropy-coded bytes: up to the first marker that is neither a stuffed 0xFF00, fill, nor RSTn (or the end of a truncated file)
            const size_t d0 = r.i;
            const size_t i = entropy_end(p, n, d0);
            if (!i) return "DNL marker is not supported";
            if (i - d0 >= JPG_MAX_DATA) return "entropy-coded data larger than 256 MiB";
            out.data = p + d0;
            out.data_len = (uint32_t)(i - d0);
            return nullptr;
        }
        default:
            break;                                   // APPn, COM, ...: skipped
        }
        r.i = seg_end;
    }
}

// ---------------------------------------------------------------------------------------------------------------- device: entropy
struct BitReader {
    const uint32_t* w;
    uint32_t nw, wi;
    uint64_t buf;
    int cnt;
    __device__ uint32_t word(uint32_t i) const { return i < nw ? __builtin_bswap32(w[i]) : 0u; }
    __device__ void refill()
    {
        if (cnt <= 32) {
            buf |= (uint64_t)word(wi) << (32 - cnt);
            ++wi;
            cnt += 32;
        }
    }
    __device__ void seek(uint32_t pos)
    {
        wi = pos >> 5;
        buf = 0;
        cnt = 0;
        refill();
        refill();
        const int s = pos & 31;
        buf <<= s;
        cnt -= s;
    }
    __device__ uint32_t pos() const { return wi * 32u - (uint32_t)cnt; }
    __device__ void skip(int n) { buf <<= n; cnt -= n; }
};

// one Huffman symbol from the top of `buf`; len 0 = no code of <= 16 bits matches
__device__ inline int huff_decode(const JHuff& t, uint64_t buf, int& len)
{
    const uint16_t e = t.lut[buf >> 55];
    if (e >> 8) {
        len = e >> 8;
        return e & 255;
    }
    const int top = (int)(buf >> 48);
    for (int l = 10; l <= 16; ++l) {
        const int code = top >> (16 - l);
        if (code <= t.maxcode[l]) {
            len = l;
            return t.huffval[(code + t.valoffset[l]) & 255];
        }
    }
    len = 0;
    return 0;
}

__device__ inline int huff_extend(int x, int s) { return x < (1 << (s - 1)) ? x + (int)(-1u << s) + 1 : x; }

// One wave removes byte stuffing and RSTn markers from `n` entropy-coded bytes, 64 bytes at a time (ballot + popcount prefix): the clean
// stream (its tail up to `clean_cap` zeroed: bits past the end read as zero), the clean-stream offsets of the interval starts
// istart[0 .. nint] (missing ones = the end), the clean length and the number of RSTn found.  The caller orders these stores before reads.
__device__ inline void destuff_wave(const uint8_t* data, uint32_t n, uint8_t* clean, uint32_t clean_cap, int* istart, int nint, int lane,
                                    uint32_t& clen, int& nrst)
{
    const uint64_t below = (1ull << lane) - 1;
    uint32_t cbase = 0;
    nrst = 0;
    for (uint32_t base = 0; base < n; base += JPG_LANES) {
        const uint32_t i = base + lane;
        bool keep = false, rst = false;
        int b = 0;
        if (i < n) {
            b = data[i];
            const int prev = i > 0 ? data[i - 1] : 0;
            const int next = i + 1 < n ? data[i + 1] : -1;
            if (b == 0xFF) keep = next == 0x00;                                  // data 0xFF; else fill or the start of RSTn
            else if (prev == 0xFF && b == 0x00) keep = false;                    // the stuffed zero
            else if (prev == 0xFF && b >= 0xD0 && b <= 0xD7) rst = true;         // RSTn
            else keep = true;
        }
        const uint64_t km = __ballot(keep), rm = __ballot(rst);
        const uint32_t at = cbase + (uint32_t)__popcll(km & below);
        if (keep) clean[at] = (uint8_t)b;
        if (rst) {
            const int j = nrst + __popcll(rm & below) + 1;
            if (j < nint) istart[j] = (int)at;
        }
        cbase += (uint32_t)__popcll(km);
        nrst += __popcll(rm);
    }
    clen = cbase;
    for (uint32_t i = clen + lane; i < clean_cap; i += JPG_LANES) clean[i] = 0;   // the last word's tail reads as zero bits
    if (lane == 0) istart[0] = 0;
    for (int j = nrst + 1 + lane; j <= nint; j += JPG_LANES) istart[j] = (int)clen;
}

struct Stretch {                 // decoding state at a symbol boundary
    uint32_t pos;
    int blk, k;
};

struct EntropyShared {
    JHuff huff[8];
    int bcomp[JPG_MAX_BPM], bdc[JPG_MAX_BPM], bac[JPG_MAX_BPM];
    uint32_t s_pos[JPG_LANES], e_pos[JPG_LANES];
    int s_blk[JPG_LANES], s_k[JPG_LANES], e_blk[JPG_LANES], e_k[JPG_LANES];
    int mcus[JPG_LANES], dcs[3][JPG_LANES];
    int status;
};

// Decodes from `st` until the stop rule: without restarts, the first symbol boundary at or past `stop` (and, when writing, the frame's
// last MCU); with restarts, MCU `mcu_end`.  Counts the MCUs completed and the DC differences per component.  WRITE: stores coefficients
// of MCU `mcu` on (natural order, into zeroed blocks) with the DC predictors `pred`.
template <bool WRITE>
__device__ void decode_stretch(const EntropyShared& sh, const JFrame& f, BitReader& br, Stretch& st, uint32_t stop, int mcu, int mcu_end,
                               const int* istart, uint32_t total_bits, int pred[3], int& mcus, int dcs[3], int16_t* coefs, int& status)
{
    br.seek(st.pos);
    const int mcu0 = mcu;
    int blk = st.blk, k = st.k;
    for (;;) {
        if (f.ri) {
            if (mcu >= mcu_end) break;
        } else {
            if (br.pos() >= stop) break;
            if (WRITE && mcu >= f.nmcu) break;
        }
        br.refill();
        const int c = sh.bcomp[blk];
        int16_t* blkp = nullptr;
        if (WRITE) {
            const JComp& cp = f.comp[c];
            int bx, by;
            if (f.ncomp == 1) {
                by = mcu / f.mcux;
                bx = mcu - by * f.mcux;
            } else {
                const int my = mcu / f.mcux;
                by = my * cp.v + f.by[blk];
                bx = (mcu - my * f.mcux) * cp.h + f.bx[blk];
            }
            blkp = coefs + ((size_t)cp.blk0 + (size_t)by * cp.bw + bx) * 64;
        }
        int len;
        if (k == 0) {
            int s = huff_decode(sh.huff[sh.bdc[blk]], br.buf, len);
            if (!len) { len = 1; s = 0; if (WRITE) status |= ST_BAD_CODE; }
            br.skip(len);
            int diff = 0;
            if (s) {
                diff = huff_extend((int)(br.buf >> (64 - s)), s);
                br.skip(s);
            }
            dcs[c] += diff;
            if (WRITE) {
                pred[c] += diff;
                blkp[0] = (int16_t)pred[c];
            }
            k = 1;
        } else {
            const int sym = huff_decode(sh.huff[sh.bac[blk]], br.buf, len);
            if (!len) {
                br.skip(1);
                if (WRITE) status |= ST_BAD_CODE;
                k = 64;                                       // a fake EOB (libjpeg fakes a zero symbol)
            } else {
                br.skip(len);
                const int rr = sym >> 4, s = sym & 15;
                if (s) {
                    k += rr;
                    if (k > 63) { k = 63; if (WRITE) status |= ST_BAD_INDEX; }
                    const int v = huff_extend((int)(br.buf >> (64 - s)), s);
                    br.skip(s);
                    if (WRITE) blkp[c_natural[k]] = (int16_t)v;
                    ++k;
                } else if (rr == 15) {
                    k += 16;
                } else {
                    k = 64;
                }
            }
        }
        if (k >= 64) {
            k = 0;
            if (++blk == f.bpm) {
                blk = 0;
                ++mcu;
                ++mcus;
                if (f.ri && mcu % f.ri == 0 && mcu < mcu_end) {   // next restart interval: byte-aligned, DC predictors reset
                    const int j = mcu / f.ri;
                    const uint32_t seg = (uint32_t)istart[j] * 8u;
                    if (WRITE && br.pos() > seg) status |= ST_TRUNCATED;
                    br.seek(seg);
                    if (WRITE) pred[0] = pred[1] = pred[2] = 0;
                }
            }
        }
    }
    if (WRITE && f.ri && mcu_end > mcu0 && mcu >= mcu_end) {      // end of this lane's last interval
        const int j = (mcu + f.ri - 1) / f.ri;
        const uint32_t seg = j < f.nint ? (uint32_t)istart[j] * 8u : total_bits;
        if (br.pos() > seg) status |= ST_TRUNCATED;
    }
    st.pos = br.pos();
    st.blk = blk;
    st.k = k;
}

__global__ void __launch_bounds__(JPG_LANES) jpeg_entropy_kernel(const uint8_t* blob, uint8_t* ws, int* status_out)
{
    const int fi = blockIdx.x;
    const int lane = threadIdx.x;
    const JFrame f = reinterpret_cast<const JFrame*>(blob + sizeof(JHeader))[fi];
    if (f.prog) return;                              // jpeg_prog_entropy_kernel's frame
    __shared__ EntropyShared sh;
    {   // tables -> LDS
        const uint32_t* src = reinterpret_cast<const uint32_t*>(blob + f.tables_off);
        uint32_t* dst = reinterpret_cast<uint32_t*>(sh.huff);
        for (int i = lane; i < (int)(sizeof(sh.huff) / 4); i += JPG_LANES) dst[i] = src[i];
        if (lane < f.bpm) {
            const int c = f.bcomp[lane];
            sh.bcomp[lane] = c;
            sh.bdc[lane] = f.comp[c].dc;
            sh.bac[lane] = f.comp[c].ac;
        }
        if (lane == 0) sh.status = 0;
    }
    // (1) byte stuffing and restart markers out: clean stream + interval starts
    uint8_t* clean = ws + f.clean_off;
    int* istart = reinterpret_cast<int*>(ws + f.istart_off);
    uint32_t clen;
    int nrst;
    destuff_wave(blob + f.data_off, f.data_len, clean, (uint32_t)f.clean_cap, istart, f.nint, lane, clen, nrst);
    __syncthreads();

    BitReader br;
    br.w = reinterpret_cast<const uint32_t*>(clean);
    br.nw = (clen + 3) / 4;
    const uint32_t total_bits = clen * 8u;
    int16_t* coefs = reinterpret_cast<int16_t*>(ws + f.coef_off);

    // (2) stretches
    Stretch st;
    uint32_t stop = 0;
    int mcu0 = 0, mcu_end = 0;
    if (f.ri) {
        const int lo = (int)((long)lane * f.nint / JPG_LANES), hi = (int)((long)(lane + 1) * f.nint / JPG_LANES);
        mcu0 = lo * f.ri;
        mcu_end = hi * f.ri < f.nmcu ? hi * f.ri : f.nmcu;
        if (mcu_end < mcu0) mcu_end = mcu0;
        st.pos = lo < f.nint ? (uint32_t)istart[lo] * 8u : total_bits;
    } else {
        st.pos = (uint32_t)((uint64_t)total_bits * lane / JPG_LANES);
        stop = lane + 1 < JPG_LANES ? (uint32_t)((uint64_t)total_bits * (lane + 1) / JPG_LANES) : total_bits;
    }
    st.blk = 0;
    st.k = 0;
    int pred[3] = {0, 0, 0};
    int my_status = lane == 0 && f.ri && nrst != f.nint - 1 ? ST_RESTART : 0;
    if (!f.ri) {
        // speculative passes until no start state changes
        const Stretch s0 = st;
        Stretch cur = s0;
        bool redo = true;
        int mcus = 0, dcs[3] = {0, 0, 0};
        for (int round = 0; round < JPG_LANES; ++round) {
            if (redo) {
                Stretch e = cur;
                mcus = 0;
                dcs[0] = dcs[1] = dcs[2] = 0;
                decode_stretch<false>(sh, f, br, e, stop, 0, 0, istart, total_bits, pred, mcus, dcs, coefs, my_status);
                sh.e_pos[lane] = e.pos; sh.e_blk[lane] = e.blk; sh.e_k[lane] = e.k;
            }
            __syncthreads();
            bool changed = false;
            if (lane > 0) {
                const uint32_t p = sh.e_pos[lane - 1];
                const int b = sh.e_blk[lane - 1], kk = sh.e_k[lane - 1];
                changed = p != cur.pos || b != cur.blk || kk != cur.k;
                cur.pos = p; cur.blk = b; cur.k = kk;
            }
            __syncthreads();
            redo = changed;
            if (!__ballot(changed)) break;
        }
        st = cur;
        // (3) wave prefix: first MCU and DC predictors of every lane
        sh.mcus[lane] = mcus;
        sh.dcs[0][lane] = dcs[0]; sh.dcs[1][lane] = dcs[1]; sh.dcs[2][lane] = dcs[2];
        __syncthreads();
        for (int j = 0; j < lane; ++j) {
            mcu0 += sh.mcus[j];
            pred[0] += sh.dcs[0][j]; pred[1] += sh.dcs[1][j]; pred[2] += sh.dcs[2][j];
        }
        if (lane == JPG_LANES - 1 && mcu0 + mcus < f.nmcu) my_status |= ST_TRUNCATED;   // the data ran out before the last MCU
        mcu_end = f.nmcu;
    }
    // (4) the writing pass
    {
        int mcus = 0, dcs[3] = {0, 0, 0};
        Stretch e = st;
        const int start_mcu = mcu0;
        decode_stretch<true>(sh, f, br, e, stop, mcu0, mcu_end, istart, total_bits, pred, mcus, dcs, coefs, my_status);
        if (!f.ri && start_mcu < f.nmcu && start_mcu + mcus >= f.nmcu && e.pos > total_bits) my_status |= ST_TRUNCATED;
    }
    if (my_status) atomicOr(&sh.status, my_status);
    __syncthreads();
    if (lane == 0) status_out[fi] = sh.status;
}

// ---------------------------------------------------------------------------------------------------------------- device: progressive
// jpeg_prog_entropy_kernel: one workgroup of JPG_PROG_WAVES waves per progressive frame.  The frame's scans are sorted by dependency level;
// the scans of one level write disjoint coefficients, so each wave takes one of them (in passes of JPG_PROG_WAVES if a level has more),
// removes its byte stuffing as the baseline kernel does, and decodes it: with restart markers every lane takes whole intervals (each
// starts in an exact state: MCU = interval * Ri, EOBRUN 0, predictors 0), without them one lane decodes the scan serially.  A batch
// supplies the parallelism here.  An AC refinement reads what earlier levels wrote into the coefficient buffer, so between passes
// stands a device-scope fence and a workgroup barrier (the barrier alone orders LDS, not global stores).
struct ProgShared {
    JHuff huff[JPG_PROG_WAVES][3];
    uint8_t natural[64];         // c_natural: the lookup stands in every symbol's dependent chain, and LDS answers sooner than memory
    int status;
};

// natural position -> zig-zag position (the inverse of c_natural), for indices known at compile time
__host__ __device__ constexpr int zigzag_of(int nat)
{
    constexpr uint8_t t[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
                               10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};
    return t[nat];
}

struct ProgBits {                // BitReader with a refill in front of every read: a scan's reads have no common rhythm
    BitReader br;
    __device__ int bit()
    {
        br.refill();
        const int b = (int)(br.buf >> 63);
        br.skip(1);
        return b;
    }
    __device__ int bits(int n)   // 1 <= n <= 16
    {
        br.refill();
        const int v = (int)(br.buf >> (64 - n));
        br.skip(n);
        return v;
    }
    __device__ int symbol(const JHuff& t, int& status)
    {
        br.refill();
        int len;
        const int s = huff_decode(t, br.buf, len);
        if (!len) {              // no such code: one bit on, a zero symbol (as libjpeg fakes one)
            br.skip(1);
            status |= ST_BAD_CODE;
            return 0;
        }
        br.skip(len);
        return s;
    }
};

// One lane: the MCUs [m, m_end) of scan `sc` (whole restart intervals), from the interval start it owns.
// `huff`: the scan's tables by scan component (an AC scan's one table at 0).
__device__ void prog_decode(const JFrame& f, const JScan& gsc, const JHuff* huff, const uint8_t* natural, ProgBits& pb, int m, int m_end,
                            const int* istart, uint32_t total_bits, int16_t* coefs, int& status)
{
    // the scan's scalars in registers: the compiler cannot keep loads of the blob across the coefficient stores
    struct { int ss, se, ah, al, ri, bpm, ncomp, mcux, nint; } sc = {gsc.ss, gsc.se > 63 ? 63 : gsc.se, gsc.ah, gsc.al & 15, gsc.ri, gsc.bpm,
                                                                    gsc.ncomp, gsc.mcux, gsc.nint};
    const int c0 = gsc.comp[0];
    const int c0_blk0 = f.comp[c0].blk0, c0_bw = f.comp[c0].bw, c0_bh = f.comp[c0].bh;
    const int m0 = m;
    int pred[3] = {0, 0, 0};
    int eobrun = 0;
    const int p1 = 1 << sc.al, m1 = -1 * (1 << sc.al);
    pb.br.seek(sc.ri ? (uint32_t)istart[m / sc.ri] * 8u : 0u);
    for (; m < m_end; ++m) {
        if (sc.ri && m > m0 && m % sc.ri == 0) {                  // next restart interval: byte-aligned, predictors and EOBRUN reset
            const uint32_t seg = (uint32_t)istart[m / sc.ri] * 8u;
            if (pb.br.pos() > seg) status |= ST_TRUNCATED;
            pb.br.seek(seg);
            pred[0] = pred[1] = pred[2] = 0;
            eobrun = 0;
        }
        for (int b = 0; b < sc.bpm; ++b) {
            int j = 0, bx, by, blk0 = c0_blk0, bw = c0_bw, bh = c0_bh;
            if (sc.ncomp == 1) {
                by = m / sc.mcux;
                bx = m - by * sc.mcux;
            } else {
                j = gsc.bcomp[b] & 3;
                j = j < 3 ? j : 2;
                const JComp& cp = f.comp[gsc.comp[j]];
                const int my = m / sc.mcux;
                by = my * cp.v + gsc.by[b];
                bx = (m - my * sc.mcux) * cp.h + gsc.bx[b];
                blk0 = cp.blk0; bw = cp.bw; bh = cp.bh;
            }
            bx = bx < bw ? bx : bw - 1;                           // in the component's blocks whatever the scan table says
            by = by < bh ? by : bh - 1;
            int16_t* blk = coefs + ((size_t)blk0 + (size_t)by * bw + bx) * 64;
            if (sc.ss == 0) {
                if (sc.ah == 0) {                                 // DC first: the difference, << Al
                    const int s = pb.symbol(huff[j], status) & 15;
                    if (s) pred[j] += huff_extend(pb.bits(s), s);
                    blk[0] = (int16_t)((uint32_t)pred[j] << sc.al);
                } else if (pb.bit()) {                            // DC refinement: one bit
                    // an atomic OR on the block's first word (coefficient 0 in its low half; the high half, coefficient 1, gets | 0 and may
                    // be stored by an AC scan of this level meanwhile): nothing comes back, so the lane does not wait for memory
                    atomicOr(reinterpret_cast<unsigned int*>(blk), (unsigned int)p1);
                }
            } else if (sc.ah == 0) {                              // AC first
                if (eobrun > 0) {
                    --eobrun;
                    continue;
                }
                for (int k = sc.ss; k <= sc.se; ++k) {
                    const int sym = pb.symbol(huff[0], status);
                    const int r = sym >> 4, s = sym & 15;
                    if (s) {
                        k += r;
                        const int v = huff_extend(pb.bits(s), s);
                        if (k > sc.se) { k = sc.se; status |= ST_BAD_INDEX; }
                        blk[natural[k]] = (int16_t)((uint32_t)v << sc.al);
                    } else if (r == 15) {
                        k += 15;
                    } else {                                      // EOBr: this block and eobrun more end here
                        eobrun = (1 << r) - 1;
                        if (r) eobrun += pb.bits(r);
                        break;
                    }
                }
            } else {                                              // AC refinement
                // the block's history as a mask over zig-zag positions (bit k: coefficient k is non-zero) from eight 16-byte loads: the
                // walk below then touches memory only where a correction bit changes a coefficient, not once per position.  A new
                // coefficient lands behind the walk (k only grows), so the mask holds for the whole block.
                uint64_t nz = 0;
                {
                    const int4* raw = reinterpret_cast<const int4*>(blk);
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        const int4 v = raw[q];
                        const uint32_t w4[4] = {(uint32_t)v.x, (uint32_t)v.y, (uint32_t)v.z, (uint32_t)v.w};
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            if (w4[i] & 0xFFFFu) nz |= 1ull << zigzag_of(q * 8 + 2 * i);
                            if (w4[i] >> 16) nz |= 1ull << zigzag_of(q * 8 + 2 * i + 1);
                        }
                    }
                }
                int k = sc.ss;
                if (eobrun == 0) {
                    for (; k <= sc.se; ++k) {
                        const int sym = pb.symbol(huff[0], status);
                        int r = sym >> 4, s = sym & 15;
                        if (s) {
                            s = pb.bit() ? p1 : m1;               // a new coefficient is +-1 << Al (a size other than 1 is corrupt data)
                        } else if (r != 15) {
                            eobrun = 1 << r;
                            if (r) eobrun += pb.bits(r);
                            break;
                        }
                        // over the coefficients with history (a correction bit each) and r without
                        for (; k <= sc.se; ++k) {
                            if (nz >> k & 1) {
                                if (pb.bit()) {
                                    const int nat = natural[k];
                                    const int v = blk[nat];
                                    if ((v & p1) == 0) blk[nat] = (int16_t)(v + (v >= 0 ? p1 : m1));
                                }
                            } else if (--r < 0) {
                                break;
                            }
                        }
                        if (s) {
                            if (k <= sc.se) blk[natural[k]] = (int16_t)s;
                            else status |= ST_BAD_INDEX;
                        }
                    }
                }
                if (eobrun > 0) {                                 // the rest of the band: correction bits only
                    for (; k <= sc.se; ++k) {
                        if ((nz >> k & 1) && pb.bit()) {
                            const int nat = natural[k];
                            const int v = blk[nat];
                            if ((v & p1) == 0) blk[nat] = (int16_t)(v + (v >= 0 ? p1 : m1));
                        }
                    }
                    --eobrun;
                }
            }
        }
    }
    if (m_end > m0) {                                             // the end of this lane's last interval
        const int jn = sc.ri ? (m_end + sc.ri - 1) / sc.ri : 1;
        const uint32_t seg = jn < sc.nint ? (uint32_t)istart[jn] * 8u : total_bits;
        if (pb.br.pos() > seg) status |= ST_TRUNCATED;
    }
}

__global__ void __launch_bounds__(JPG_PROG_WAVES * JPG_LANES) jpeg_prog_entropy_kernel(const uint8_t* __restrict__ blob, uint8_t* ws,
                                                                                       int* status_out)
{
    const int fi = blockIdx.x;
    const int lane = threadIdx.x & (JPG_LANES - 1), wave = threadIdx.x / JPG_LANES;
    const JHeader& hd = *reinterpret_cast<const JHeader*>(blob);
    const JFrame& f = reinterpret_cast<const JFrame*>(blob + sizeof(JHeader))[fi];
    if (!f.prog) return;                             // jpeg_entropy_kernel's frame
    const JProg pg = reinterpret_cast<const JProg*>(blob + hd.prog_off)[fi];
    const JScan* scans = reinterpret_cast<const JScan*>(blob + pg.scans_off);
    const JHuff* huffs = reinterpret_cast<const JHuff*>(blob + pg.huff_off);
    int16_t* coefs = reinterpret_cast<int16_t*>(ws + f.coef_off);
    __shared__ ProgShared sh;
    if (threadIdx.x == 0) sh.status = 0;
    if (threadIdx.x < 64) sh.natural[threadIdx.x] = c_natural[threadIdx.x];
    int my_status = 0;
    int s = 0;
    while (s < pg.nscan) {                           // one level (uniform over the workgroup: the scan table is read-only)
        const int level = scans[s].level;
        int e = s + 1;
        while (e < pg.nscan && scans[e].level == level) ++e;
        for (int s0 = s; s0 < e; s0 += JPG_PROG_WAVES) {
            const int si = s0 + wave;
            const bool active = si < e;
            uint32_t clen = 0;
            int nrst = 0;
            if (active) {
                const JScan& sc = scans[si];
                for (int j = 0; j < sc.ncomp; ++j) {
                    if (sc.tab[j] < 0 || sc.tab[j] >= pg.nhuff) continue;
                    const uint32_t* src = reinterpret_cast<const uint32_t*>(huffs + sc.tab[j]);
                    uint32_t* dst = reinterpret_cast<uint32_t*>(&sh.huff[wave][j]);
                    for (int i = lane; i < (int)(sizeof(JHuff) / 4); i += JPG_LANES) dst[i] = src[i];
                }
                destuff_wave(blob + sc.data_off, sc.data_len, ws + sc.clean_off, (uint32_t)sc.clean_cap,
                             reinterpret_cast<int*>(ws + sc.istart_off), sc.nint, lane, clen, nrst);
            }
            // the clean streams, and the coefficients of the levels before, become visible to every wave of the workgroup
            __threadfence();
            __syncthreads();
            if (active) {
                const JScan& sc = scans[si];
                const int* istart = reinterpret_cast<const int*>(ws + sc.istart_off);
                if (lane == 0 && sc.ri && nrst != sc.nint - 1) my_status |= ST_RESTART;
                if (lane == 0 && !sc.ri && nrst) my_status |= ST_RESTART;
                const int lo = (int)((long)lane * sc.nint / JPG_LANES), hi = (int)((long)(lane + 1) * sc.nint / JPG_LANES);
                int m = 0, m_end = 0;
                if (hi > lo) {
                    m = sc.ri ? lo * sc.ri : 0;
                    m_end = sc.ri && (long)hi * sc.ri < sc.nmcu ? hi * sc.ri : sc.nmcu;
                }
                if (m_end > m) {
                    ProgBits pb;
                    pb.br.w = reinterpret_cast<const uint32_t*>(ws + sc.clean_off);
                    pb.br.nw = (clen + 3) / 4;
                    prog_decode(f, sc, sh.huff[wave], sh.natural, pb, m, m_end, istart, clen * 8u, coefs, my_status);
                }
            }
        }
        s = e;
    }
    if (my_status) atomicOr(&sh.status, my_status);
    __syncthreads();
    if (threadIdx.x == 0) status_out[fi] = sh.status;
}

// ---------------------------------------------------------------------------------------------------------------- device: IDCT
constexpr int64_t FIX_0_298631336 = 2446, FIX_0_390180644 = 3196, FIX_0_541196100 = 4433, FIX_0_765366865 = 6270, FIX_0_899976223 = 7373,
                  FIX_1_175875602 = 9633, FIX_1_501321110 = 12299, FIX_1_847759065 = 15137, FIX_1_961570560 = 16069,
                  FIX_2_053119869 = 16819, FIX_2_562915447 = 20995, FIX_3_072711026 = 25172;
constexpr int CONST_BITS = 13, PASS1_BITS = 2;

__device__ inline int64_t descale(int64_t x, int n) { return (x + ((int64_t)1 << (n - 1))) >> n; }

// libjpeg's idct_sample_range_limit[x & 0x3FF]: x + 128 clamped to [0, 255] for x in [-512, 511], wrapping beyond
__device__ inline uint32_t idct_range(int64_t v)
{
    const int x = (int)(v & 0x3FF);
    return x < 128 ? x + 128 : x < 512 ? 255 : x < 896 ? 0 : x - 896;
}

// jpeg_idct_islow's even / odd butterfly on 8 inputs (in[0..7] = the samples at 0 .. 7 of one column or row)
__device__ inline void islow_1d(const int64_t in[8], int64_t out_hi[4], int64_t out_odd[4])
{
    int64_t z2 = in[2], z3 = in[6];
    int64_t z1 = (z2 + z3) * FIX_0_541196100;
    const int64_t tmp2 = z1 + z3 * -FIX_1_847759065;
    const int64_t tmp3 = z1 + z2 * FIX_0_765366865;
    z2 = in[0];
    z3 = in[4];
    const int64_t t0 = (z2 + z3) * (1 << CONST_BITS);
    const int64_t t1 = (z2 - z3) * (1 << CONST_BITS);
    out_hi[0] = t0 + tmp3;   // tmp10
    out_hi[3] = t0 - tmp3;   // tmp13
    out_hi[1] = t1 + tmp2;   // tmp11
    out_hi[2] = t1 - tmp2;   // tmp12
    int64_t o0 = in[7], o1 = in[5], o2 = in[3], o3 = in[1];
    z1 = o0 + o3;
    z2 = o1 + o2;
    z3 = o0 + o2;
    int64_t z4 = o1 + o3;
    const int64_t z5 = (z3 + z4) * FIX_1_175875602;
    o0 *= FIX_0_298631336;
    o1 *= FIX_2_053119869;
    o2 *= FIX_3_072711026;
    o3 *= FIX_1_501321110;
    z1 *= -FIX_0_899976223;
    z2 *= -FIX_2_562915447;
    z3 *= -FIX_1_961570560;
    z4 *= -FIX_0_390180644;
    z3 += z5;
    z4 += z5;
    out_odd[0] = o0 + z1 + z3;
    out_odd[1] = o1 + z2 + z4;
    out_odd[2] = o2 + z2 + z3;
    out_odd[3] = o3 + z1 + z4;
}

__global__ void __launch_bounds__(256) jpeg_idct_kernel(const uint8_t* blob, uint8_t* ws)
{
    const JFrame& f = reinterpret_cast<const JFrame*>(blob + sizeof(JHeader))[blockIdx.y];
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= f.nblocks) return;
    int c = 0;
    while (c + 1 < f.ncomp && b >= f.comp[c + 1].blk0) ++c;
    const JComp& cp = f.comp[c];
    const int local = b - cp.blk0;
    const int by = local / cp.bw, bx = local - by * cp.bw;
    const uint16_t* q = reinterpret_cast<const JTables*>(blob + f.tables_off)->q[cp.q];
    const int4* src = reinterpret_cast<const int4*>(ws + f.coef_off + (size_t)b * 128);
    int16_t coef[64];
    for (int i = 0; i < 8; ++i) *reinterpret_cast<int4*>(coef + 8 * i) = src[i];
    int ws_[64];
    for (int col = 0; col < 8; ++col) {                      // pass 1: columns
        int64_t in[8];
        for (int r = 0; r < 8; ++r) in[r] = (int64_t)((int)coef[r * 8 + col] * (int)q[r * 8 + col]);
        int64_t e[4], o[4];
        islow_1d(in, e, o);
        const int sh = CONST_BITS - PASS1_BITS;
        ws_[0 * 8 + col] = (int)descale(e[0] + o[3], sh);
        ws_[7 * 8 + col] = (int)descale(e[0] - o[3], sh);
        ws_[1 * 8 + col] = (int)descale(e[1] + o[2], sh);
        ws_[6 * 8 + col] = (int)descale(e[1] - o[2], sh);
        ws_[2 * 8 + col] = (int)descale(e[2] + o[1], sh);
        ws_[5 * 8 + col] = (int)descale(e[2] - o[1], sh);
        ws_[3 * 8 + col] = (int)descale(e[3] + o[0], sh);
        ws_[4 * 8 + col] = (int)descale(e[3] - o[0], sh);
    }
    const int stride = cp.bw * 8;
    uint8_t* dst = ws + cp.plane_off + (size_t)by * 8 * stride + (size_t)bx * 8;
    for (int r = 0; r < 8; ++r) {                            // pass 2: rows
        int64_t in[8];
        for (int i = 0; i < 8; ++i) in[i] = ws_[r * 8 + i];
        int64_t e[4], o[4];
        islow_1d(in, e, o);
        const int sh = CONST_BITS + PASS1_BITS + 3;
        uint32_t px[8];
        px[0] = idct_range(descale(e[0] + o[3], sh));
        px[7] = idct_range(descale(e[0] - o[3], sh));
        px[1] = idct_range(descale(e[1] + o[2], sh));
        px[6] = idct_range(descale(e[1] - o[2], sh));
        px[2] = idct_range(descale(e[2] + o[1], sh));
        px[5] = idct_range(descale(e[2] - o[1], sh));
        px[3] = idct_range(descale(e[3] + o[0], sh));
        px[4] = idct_range(descale(e[3] - o[0], sh));
        uint2 v;
        v.x = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
        v.y = px[4] | (px[5] << 8) | (px[6] << 16) | (px[7] << 24);
        *reinterpret_cast<uint2*>(dst + (size_t)r * stride) = v;
    }
}

// ---------------------------------------------------------------------------------------------------------------- device: colour
__device__ inline int plane_at(const uint8_t* p, int stride, int y, int x) { return p[(size_t)y * stride + x]; }

// chroma sample at output pixel (y, x) for luma sampling (H, V): libjpeg-turbo's upsamplers (jdsample.c)
__device__ inline int upsample(const uint8_t* p, const JComp& cp, int H, int V, int y, int x)
{
    const int stride = cp.bw * 8;
    if (H == 1 && V == 1) return plane_at(p, stride, y, x);
    if (H == 2 && V == 1) {
        const int j = x >> 1;
        if (cp.dw <= 2) return plane_at(p, stride, y, j);
        const int c = plane_at(p, stride, y, j) * 3;
        return (x & 1) ? (c + plane_at(p, stride, y, j + 1 < cp.dw ? j + 1 : j) + 2) >> 2
                       : (c + plane_at(p, stride, y, j > 0 ? j - 1 : 0) + 1) >> 2;
    }
    const int i = y >> 1;
    const int n = (y & 1) ? (i + 1 < cp.dh ? i + 1 : i) : (i > 0 ? i - 1 : 0);
    if (H == 1) return (plane_at(p, stride, i, x) * 3 + plane_at(p, stride, n, x) + ((y & 1) ? 2 : 1)) >> 2;   // h1v2
    const int j = x >> 1;
    if (cp.dw <= 2) return plane_at(p, stride, i, j);                                                             // h2v2_upsample
    const int cs = plane_at(p, stride, i, j) * 3 + plane_at(p, stride, n, j);
    const int jj = (x & 1) ? (j + 1 < cp.dw ? j + 1 : j) : (j > 0 ? j - 1 : 0);
    const int cs2 = plane_at(p, stride, i, jj) * 3 + plane_at(p, stride, n, jj);
    return (x & 1) ? (cs * 3 + cs2 + 7) >> 4 : (cs * 3 + cs2 + 8) >> 4;
}

__device__ inline uint32_t clamp255(int v) { return v < 0 ? 0u : v > 255 ? 255u : (uint32_t)v; }

// one pixel -> B | G << 8 | R << 16
__device__ inline uint32_t pixel_bgr(const uint8_t* ws, const JFrame& f, int y, int x)
{
    const JComp& c0 = f.comp[0];
    const int yv = plane_at(ws + c0.plane_off, c0.bw * 8, y, x);
    if (f.ncomp == 1) return yv | (yv << 8) | (yv << 16);
    const int a = upsample(ws + f.comp[1].plane_off, f.comp[1], c0.h, c0.v, y, x);
    const int b = upsample(ws + f.comp[2].plane_off, f.comp[2], c0.h, c0.v, y, x);
    if (f.color == 2) return (uint32_t)b | ((uint32_t)a << 8) | ((uint32_t)yv << 16);
    // ycc_rgb_convert (jdcolor.c): SCALEBITS 16, ONE_HALF 1 << 15, tables of build_ycc_rgb_table
    const int cb = a - 128, cr = b - 128;
    const int r_add = (int)((91881LL * cr + 32768) >> 16);
    const int b_add = (int)((116130LL * cb + 32768) >> 16);
    const int g_add = (int)((-46802LL * cr + (-22554LL * cb + 32768)) >> 16);
    return clamp255(yv + b_add) | (clamp255(yv + g_add) << 8) | (clamp255(yv + r_add) << 16);
}

__global__ void __launch_bounds__(256) jpeg_color_kernel(const uint8_t* blob, const uint8_t* ws, uint8_t* bgr)
{
    const JHeader& hd = *reinterpret_cast<const JHeader*>(blob);
    const JFrame* frames = reinterpret_cast<const JFrame*>(blob + sizeof(JHeader));
    const long hw = (long)hd.h * hd.w;
    const long npix = hw * hd.n;
    const long p0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (p0 >= npix) return;
    uint32_t px[4];
    const int m = npix - p0 < 4 ? (int)(npix - p0) : 4;
    for (int i = 0; i < m; ++i) {
        const long p = p0 + i;
        const int fi = (int)(p / hw);
        const int r = (int)(p - (long)fi * hw);
        const int y = r / hd.w, x = r - y * hd.w;
        px[i] = pixel_bgr(ws, frames[fi], y, x);
    }
    uint8_t* out = bgr + p0 * 3;
    if (m == 4) {
        uint32_t* o = reinterpret_cast<uint32_t*>(out);
        o[0] = (px[0] & 0xFFFFFF) | (px[1] << 24);
        o[1] = ((px[1] >> 8) & 0xFFFF) | (px[2] << 16);
        o[2] = ((px[2] >> 16) & 0xFF) | (px[3] << 8);
    } else {
        for (int i = 0; i < m; ++i) {
            out[3 * i] = (uint8_t)px[i];
            out[3 * i + 1] = (uint8_t)(px[i] >> 8);
            out[3 * i + 2] = (uint8_t)(px[i] >> 16);
        }
    }
}

const JHeader* header_of(const void* host_blob)
{
    const JHeader* hd = static_cast<const JHeader*>(host_blob);
    return hd && hd->magic == JPG_MAGIC && hd->version == JPG_VERSION && hd->n > 0 ? hd : nullptr;
}

}  // namespace

extern "C" {

int yf_jpeg_pack(int n, const void* const* files, const size_t* nbytes, void* host_blob, size_t blob_cap, size_t* blob_bytes, int* h, int* w)
{
    return yf_jpeg_pack_ex(n, files, nbytes, 0, host_blob, blob_cap, blob_bytes, h, w);
}

int yf_jpeg_pack_ex(int n, const void* const* files, const size_t* nbytes, int flags, void* host_blob, size_t blob_cap, size_t* blob_bytes,
                    int* h, int* w)
{
    if (n <= 0 || n > 65535 || !files || !nbytes || !blob_bytes) return fail(YF_E_INVALID, "yf_jpeg_pack: n not in 1 .. 65535 or null pointer");
    if (flags & ~YF_JPEG_PROGRESSIVE) return fail(YF_E_INVALID, "yf_jpeg_pack_ex: unknown flag in 0x%x", flags);
    std::vector<Parsed> fr(n);
    for (int i = 0; i < n; ++i) {
        if (!files[i]) return fail(YF_E_INVALID, "frame %d: null file pointer", i);
        const char* why = parse_file(static_cast<const uint8_t*>(files[i]), nbytes[i], fr[i], flags);
        if (why) return fail(YF_E_INVALID, "frame %d: %s", i, why);
        if (fr[i].h != fr[0].h || fr[i].w != fr[0].w)
            return fail(YF_E_INVALID, "frame %d: %dx%d differs from frame 0's %dx%d (one call decodes frames of one size)", i, fr[i].w, fr[i].h,
                        fr[0].w, fr[0].h);
    }
    // blob: header, descriptors, tables, entropy bytes; workspace: clean streams + interval starts, coefficients, planes
    uint64_t off = align_up(sizeof(JHeader) + sizeof(JFrame) * (size_t)n, 256);
    for (auto& p : fr) { p.f.tables_off = off; off += align_up(sizeof(JTables), 256); }
    for (auto& p : fr) { p.f.data_off = off; p.f.data_len = p.data_len; off += align_up(p.data_len, 256); }
    // progressive frames: JProg[n], then per frame its scan table, table snapshots and the scans' bytes
    int nprog = 0;
    for (auto& p : fr) nprog += p.f.prog;
    const uint64_t prog_off = nprog ? off : 0;
    std::vector<JProg> pg(n);
    memset(pg.data(), 0, sizeof(JProg) * n);
    if (nprog) {
        off = align_up(off + sizeof(JProg) * (size_t)n, 256);
        for (int i = 0; i < n; ++i) {
            Parsed& p = fr[i];
            if (!p.f.prog) continue;
            pg[i].nscan = (int)p.scans.size();
            pg[i].nlevel = p.nlevel;
            pg[i].nhuff = (int)p.huffs.size();
            pg[i].scans_off = off;
            off = align_up(off + sizeof(JScan) * p.scans.size(), 256);
            pg[i].huff_off = off;
            off = align_up(off + sizeof(JHuff) * p.huffs.size(), 256);
            for (auto& sc : p.scans) { sc.data_off = off; off += align_up(sc.data_len, 256); }
        }
    }
    const uint64_t total = off;
    uint64_t wso = 0;
    for (auto& p : fr) {
        for (auto& sc : p.scans) {
            sc.clean_off = wso;
            sc.clean_cap = align_up(sc.data_len, 4) + 8;
            wso = align_up(wso + sc.clean_cap, 256);
            sc.istart_off = wso;
            wso = align_up(wso + 4 * (uint64_t)(sc.nint + 1), 256);
        }
        if (p.f.prog) continue;
        p.f.clean_off = wso;
        p.f.clean_cap = align_up(p.data_len, 4) + 8;
        wso = align_up(wso + p.f.clean_cap, 256);
        p.f.istart_off = wso;
        wso = align_up(wso + 4 * (uint64_t)(p.f.nint + 1), 256);
    }
    const uint64_t coef_begin = wso;
    int max_blocks = 0;
    for (auto& p : fr) {
        p.f.coef_off = wso;
        wso = align_up(wso + 128 * (uint64_t)p.f.nblocks, 256);
        if (p.f.nblocks > max_blocks) max_blocks = p.f.nblocks;
    }
    const uint64_t coef_end = wso;
    for (auto& p : fr)
        for (int c = 0; c < p.f.ncomp; ++c) {
            p.f.comp[c].plane_off = wso;
            wso = align_up(wso + 64 * (uint64_t)p.f.comp[c].bw * p.f.comp[c].bh, 256);
        }
    *blob_bytes = total;
    if (h) *h = fr[0].h;
    if (w) *w = fr[0].w;
    if (!host_blob) return YF_OK;
    if (blob_cap < total) return fail(YF_E_INVALID, "yf_jpeg_pack: blob capacity %zu B < %zu B", blob_cap, (size_t)total);
    uint8_t* b = static_cast<uint8_t*>(host_blob);
    JHeader hd{};
    hd.magic = JPG_MAGIC;
    hd.n = n;
    hd.h = fr[0].h;
    hd.w = fr[0].w;
    hd.blob_bytes = total;
    hd.ws_bytes = wso;
    hd.coef_begin = coef_begin;
    hd.coef_end = coef_end;
    hd.max_blocks = max_blocks;
    hd.version = JPG_VERSION;
    hd.nprog = nprog;
    hd.prog_off = prog_off;
    memset(b, 0, align_up(sizeof(JHeader) + sizeof(JFrame) * (size_t)n, 256));
    memcpy(b, &hd, sizeof hd);
    for (int i = 0; i < n; ++i) {
        memcpy(b + sizeof(JHeader) + sizeof(JFrame) * i, &fr[i].f, sizeof(JFrame));
        memcpy(b + fr[i].f.tables_off, &fr[i].t, sizeof(JTables));
        if (fr[i].data_len) memcpy(b + fr[i].f.data_off, fr[i].data, fr[i].data_len);
    }
    if (nprog) {
        memcpy(b + prog_off, pg.data(), sizeof(JProg) * n);
        for (int i = 0; i < n; ++i) {
            const Parsed& p = fr[i];
            if (!p.f.prog) continue;
            memcpy(b + pg[i].scans_off, p.scans.data(), sizeof(JScan) * p.scans.size());
            if (!p.huffs.empty()) memcpy(b + pg[i].huff_off, p.huffs.data(), sizeof(JHuff) * p.huffs.size());
            for (size_t s = 0; s < p.scans.size(); ++s)
                if (p.scans[s].data_len) memcpy(b + p.scans[s].data_off, p.sdata[s], p.scans[s].data_len);
        }
    }
    return YF_OK;
}

int yf_jpeg_workspace_bytes(const void* host_blob, size_t* bytes)
{
    const JHeader* hd = header_of(host_blob);
    if (!hd || !bytes) return fail(YF_E_INVALID, "yf_jpeg_workspace_bytes: not a blob of yf_jpeg_pack");
    *bytes = hd->ws_bytes;
    return YF_OK;
}

int yf_jpeg_frame_info(const void* host_blob, int frame, int* info, int n_info)
{
    const JHeader* hd = header_of(host_blob);
    if (!hd || !info || frame < 0 || frame >= hd->n || n_info < 25) return fail(YF_E_INVALID, "yf_jpeg_frame_info: bad argument");
    const JFrame& f = reinterpret_cast<const JFrame*>(hd + 1)[frame];
    const int head[7] = {f.ncomp, f.color, f.mcux, f.mcuy, f.nmcu, f.bpm, f.ri};
    memcpy(info, head, sizeof head);
    for (int c = 0; c < 3; ++c) {
        const JComp& k = f.comp[c];
        const int v[6] = {k.h, k.v, k.bw, k.bh, k.dw, k.dh};
        for (int j = 0; j < 6; ++j) info[7 + 6 * c + j] = c < f.ncomp ? v[j] : 0;
    }
    return YF_OK;
}

// The scan (file order) of a progressive frame, or null.
const JScan* scan_of(const JHeader* hd, int frame, int scan, int* nscan, int* nlevel)
{
    const uint8_t* b = reinterpret_cast<const uint8_t*>(hd);
    const JFrame& f = reinterpret_cast<const JFrame*>(hd + 1)[frame];
    *nscan = *nlevel = 0;
    if (!f.prog || !hd->nprog) return nullptr;
    const JProg& pg = reinterpret_cast<const JProg*>(b + hd->prog_off)[frame];
    *nscan = pg.nscan;
    *nlevel = pg.nlevel;
    const JScan* sc = reinterpret_cast<const JScan*>(b + pg.scans_off);
    for (int s = 0; s < pg.nscan; ++s)
        if (sc[s].index == scan) return sc + s;
    return nullptr;
}

int yf_jpeg_scan_info(const void* host_blob, int frame, int scan, int* info, int n_info)
{
    const JHeader* hd = header_of(host_blob);
    if (!hd || !info || frame < 0 || frame >= hd->n || n_info < 12) return fail(YF_E_INVALID, "yf_jpeg_scan_info: bad argument");
    int nscan, nlevel;
    const JScan* sc = scan_of(hd, frame, scan, &nscan, &nlevel);
    memset(info, 0, sizeof(int) * 12);
    info[0] = nscan;
    info[1] = nlevel;
    if (!nscan) return YF_OK;                      // a baseline frame
    if (!sc) return fail(YF_E_INVALID, "yf_jpeg_scan_info: frame %d has scans 0 .. %d", frame, nscan - 1);
    int mask = 0;
    for (int j = 0; j < sc->ncomp; ++j) mask |= 1 << sc->comp[j];
    const int v[10] = {sc->ncomp, mask, sc->ss, sc->se, sc->ah, sc->al, sc->level, (int)sc->file_off, (int)sc->data_len, sc->ri};
    memcpy(info + 2, v, sizeof v);
    return YF_OK;
}

int yf_jpeg_huff_lookup(const void* host_blob, int frame, int table, unsigned bits16, int* length, int* symbol)
{
    return yf_jpeg_huff_lookup_ex(host_blob, frame, -1, table, bits16, length, symbol);
}

int yf_jpeg_huff_lookup_ex(const void* host_blob, int frame, int scan, int table, unsigned bits16, int* length, int* symbol)
{
    const JHeader* hd = header_of(host_blob);
    if (!hd || frame < 0 || frame >= hd->n || table < 0 || table > 7 || !length || !symbol)
        return fail(YF_E_INVALID, "yf_jpeg_huff_lookup: bad argument");
    const JFrame& f = reinterpret_cast<const JFrame*>(hd + 1)[frame];
    const JHuff* tp = &reinterpret_cast<const JTables*>(static_cast<const uint8_t*>(host_blob) + f.tables_off)->huff[table];
    if (scan >= 0) {                               // the snapshot scan `scan` of a progressive frame took of table `table`
        int nscan, nlevel;
        const JScan* sc = scan_of(hd, frame, scan, &nscan, &nlevel);
        tp = nullptr;
        for (int j = 0; sc && j < sc->ncomp; ++j)
            if (sc->tid[j] == table) {
                const JProg& pg = reinterpret_cast<const JProg*>(static_cast<const uint8_t*>(host_blob) + hd->prog_off)[frame];
                tp = reinterpret_cast<const JHuff*>(static_cast<const uint8_t*>(host_blob) + pg.huff_off) + sc->tab[j];
            }
        if (!tp) return fail(YF_E_INVALID, "yf_jpeg_huff_lookup_ex: scan %d of frame %d does not use table %d", scan, frame, table);
    }
    const JHuff& t = *tp;
    const uint64_t buf = (uint64_t)(bits16 & 0xFFFF) << 48;
    // the device's huff_decode
    const uint16_t e = t.lut[buf >> 55];
    *length = 0;
    *symbol = 0;
    if (e >> 8) {
        *length = e >> 8;
        *symbol = e & 255;
        return YF_OK;
    }
    const int top = (int)(buf >> 48);
    for (int l = 10; l <= 16; ++l) {
        const int code = top >> (16 - l);
        if (code <= t.maxcode[l]) {
            *length = l;
            *symbol = t.huffval[(code + t.valoffset[l]) & 255];
            break;
        }
    }
    return YF_OK;
}

int yf_jpeg_decode_u8(int device, const void* host_blob, const void* d_blob, void* d_workspace, size_t ws_bytes, uint8_t* d_bgr, int* d_status,
                      void* stream)
{
    const JHeader* hd = header_of(host_blob);
    if (!hd || !d_blob || !d_bgr || !d_status) return fail(YF_E_INVALID, "yf_jpeg_decode_u8: null pointer or not a blob of yf_jpeg_pack");
    if (hd->n > 65535) return fail(YF_E_INVALID, "yf_jpeg_decode_u8: more than 65535 frames in one call");
    if (!d_workspace || ws_bytes < hd->ws_bytes) return fail(YF_E_WORKSPACE, "workspace %zu B < required %zu B", ws_bytes, (size_t)hd->ws_bytes);
    if ((uintptr_t)d_bgr % 4 || (uintptr_t)d_blob % 256 || (uintptr_t)d_workspace % 256)
        return fail(YF_E_INVALID, "yf_jpeg_decode_u8: output must be 4-byte aligned, blob and workspace 256-byte aligned");
    HIP_OK(hipSetDevice(device));
    const hipStream_t s = (hipStream_t)stream;
    const uint8_t* blob = static_cast<const uint8_t*>(d_blob);
    uint8_t* ws = static_cast<uint8_t*>(d_workspace);
    HIP_OK(hipMemsetAsync(ws + hd->coef_begin, 0, hd->coef_end - hd->coef_begin, s));
    if (hd->nprog < hd->n) hipLaunchKernelGGL(jpeg_entropy_kernel, dim3(hd->n), dim3(JPG_LANES), 0, s, blob, ws, d_status);
    if (hd->nprog) hipLaunchKernelGGL(jpeg_prog_entropy_kernel, dim3(hd->n), dim3(JPG_PROG_WAVES * JPG_LANES), 0, s, blob, ws, d_status);
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((hd->max_blocks + 255) / 256, hd->n), dim3(256), 0, s, blob, ws);
    const long quads = ((long)hd->n * hd->h * hd->w + 3) / 4;
    hipLaunchKernelGGL(jpeg_color_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, s, blob, (const uint8_t*)ws, d_bgr);
    HIP_OK(hipGetLastError());
    return YF_OK;
}

}  // extern "C"
